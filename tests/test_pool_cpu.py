"""CPU: K15 without a device -- the numpy restatement of the pooling against the reference's own compute_correspondence
(tests/golden/g10_pool.npz, made by tests/golden/make_golden_pool.py), the cameras and the mesh normalisation against what the
reference handed its renderer, the depth-to-image expression against the images it fed its network, the tie rule of the vertex
ids, and the argument checks of the two entry points (they come before any HIP call: device pointers are dummy non-null
integers that nothing dereferences)."""
import ctypes
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import pool_np as PN
import render_np as R
from dynamicfusion_body_amd import _lib, build, descriptors

OK, BADARG = 0, -1
PTR = 0x1000                                    # a "device pointer" (16-byte aligned)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_pool.npz")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def golden_inputs():
    vid = np.stack([PN.golden_ids(v) for v in range(PN.G_VIEWS)])
    feats = np.stack([PN.golden_features(v) for v in range(PN.G_VIEWS)])
    return vid, feats


def on_own_thread(test):
    """dfh_last_error() is kept per thread: the refused calls are made on a thread of their own."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        with ThreadPoolExecutor(1) as ex:
            return ex.submit(test, *args, **kwargs).result()
    return run


# ---- the reference golden ------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_reference_bit_for_bit(golden, golden_inputs):
    vid, feats = golden_inputs
    feat, cnt = PN.pool_features(vid, feats, PN.G_VERTS)
    assert golden["feat"].dtype == np.float32 and golden["feat"].shape == (PN.G_VERTS, PN.G_DIM)
    assert (cnt > 200).all()
    assert np.array_equal(feat.view(np.uint32), golden["feat"].view(np.uint32))
    # the fixture can see a wrong order
    down, cnt_down = PN.pool_features(vid, feats, PN.G_VERTS, descending=True)
    assert np.array_equal(cnt, cnt_down)
    assert (down.view(np.uint32) != golden["feat"].view(np.uint32)).any()


def test_vectorised_restatement_is_the_loop():
    rng = np.random.default_rng(3)
    vid = rng.integers(-2, 9, size=(5, 41)).astype(np.int32)         # -2, -1, 7 and 8 are no vertex of 7
    feats = (rng.standard_normal((5, 41, 3)) * 10.0 ** rng.integers(-3, 8, size=(5, 41, 3))).astype(np.float32)
    a, ca = PN.pool_features(vid, feats, 7)
    b, cb = PN.pool_features_loop(vid, feats, 7)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ca, cb)
    assert ca.sum() == ((vid >= 0) & (vid < 7)).sum()


def _clip_rows(mvp, P):
    """fp64 clip x, y, w of points P under one of the reference's mvp matrices."""
    M = mvp.astype(np.float64)
    Ph = np.concatenate([P, np.ones((len(P), 1))], axis=1)
    return Ph @ M[0], Ph @ M[1], Ph @ M[3]


def test_turntable_views_are_the_references_cameras(golden):
    K, lws = descriptors.turntable_views()
    assert K.shape == (3, 3) and lws.shape == (PN.G_VIEWS, 3, 4) and golden["mvp"].shape == (PN.G_VIEWS, 4, 4)
    P = golden["vbuf"]
    W, H = PN.G_W, PN.G_H
    for vi in range(PN.G_VIEWS):
        cx, cy, cw = _clip_rows(golden["mvp"][vi], P)
        want_u = (W - 1) / 2.0 - (W / 2.0) * (cx / cw)
        want_v = (H - 1) / 2.0 - (H / 2.0) * (cy / cw)
        u, v, z = R.project(P, K, lws[vi], 1.0, 0.0, 0.0)
        assert (cw > 1.0).all() and (cw < 3.5).all()                  # the regularised body sits inside the depth range
        np.testing.assert_allclose(u, want_u, rtol=1e-9, atol=0)
        np.testing.assert_allclose(v, want_v, rtol=1e-9, atol=0)
        np.testing.assert_allclose(z, cw, rtol=1e-9, atol=0)
    # the options move the cameras: another image size, distance and step
    K2, lws2 = descriptors.turntable_views(width=128, height=96, dis=250, step_deg=30)
    assert lws2.shape == (12, 3, 4) and K2[0, 2] == 63.5 and K2[1, 2] == 47.5 and K2[0, 0] == -64.0 and K2[1, 1] == -48.0
    assert np.allclose(lws2[0][2, 3], 2.5)


def test_regularize_mesh_is_the_references(golden):
    verts, faces = PN.golden_mesh()
    before = verts.copy()
    reg = descriptors.regularize_mesh(verts)
    assert np.array_equal(verts, before)                              # the caller's array is left alone
    assert np.abs(reg[faces.reshape(-1)] - golden["vbuf"]).max() <= 1e-12
    assert abs((reg[:, 1].max() - reg[:, 1].min()) - 1.8) <= 1e-12 and np.abs(reg.mean(axis=0)).max() <= 1e-12
    flipped = descriptors.regularize_mesh(verts, flipyz=True)
    assert np.array_equal(verts, before)
    assert abs((flipped[:, 1].max() - flipped[:, 1].min()) - 1.8) <= 1e-12
    swapped = descriptors.regularize_mesh(verts[:, [0, 2, 1]])
    assert np.array_equal(flipped, swapped)
    with pytest.raises(ValueError):
        descriptors.regularize_mesh(np.zeros((0, 3)))


def test_image_expression_is_within_one_grey_level_of_the_references(golden):
    assert golden["images"].shape == (PN.G_VIEWS, PN.G_H, PN.G_W) and golden["images"].dtype == np.uint8
    differ = lit = 0
    for vi in range(PN.G_VIEWS):
        d = PN.golden_depth_from_z(PN.golden_z(vi))
        mine = PN.image_from_depth(d.astype(np.float32), PN.G_ZNEAR, PN.G_ZFAR)
        ref = golden["images"][vi]
        assert np.abs(mine.astype(np.int32) - ref.astype(np.int32)).max() <= 1
        on = ref > 0
        lit += int(on.sum())
        differ += int((mine != ref).sum())
        assert (mine[PN.golden_z(vi) == 1.0] == 0).all()              # the far plane is the background: 0 in both
    assert lit > 20000                                                # the images are not empty
    print("image expression: %d of %d lit pixels differ by one grey level (%.3f %%)" % (differ, lit, 100.0 * differ / lit))


def test_image_expression_edges():
    f = PN.image_from_depth
    d = np.array([1.0, 3.5, 0.999999, 3.5000002, np.nan, np.inf, -1.0, 2.25, 1.0098], dtype=np.float32)
    assert f(d, 1.0, 3.5).tolist() == [255, 0, 0, 0, 0, 0, 0, 127, 254]


# ---- the tie rule ----------------------------------------------------------------------------------------------------------------------
TIE_K = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
TIE_LW = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])


def tie_triangle():
    """Integer pixel corners (2, 2), (14, 2), (8, 14) at depth 2 (u = 2 x / 2: the vertices sit at x = 2 u): the centroid
    (8, 6), the edge midpoints (8, 2), (11, 8), (5, 8) are pixel centres, and every edge value there is an exact integer."""
    verts = np.array([[4.0, 4.0, 2.0], [28.0, 4.0, 2.0], [16.0, 28.0, 2.0]])
    return verts, np.array([[0, 1, 2]], dtype=np.int32)


def test_tie_rule():
    verts, faces = tie_triangle()
    vid, image = PN.vertex_ids(verts, faces, TIE_K, TIE_LW, 16, 16, 1.0, 3.5)
    vid, image = vid[0], image[0]
    assert vid[6, 8] == 2                                             # three-way tie at the centroid: corner 2
    assert vid[2, 8] == 1                                             # 0/1 tie on the midpoint of edge 01: corner 1
    assert vid[8, 11] == 2                                            # 1/2 tie: corner 2
    assert vid[8, 5] == 2                                             # 0/2 tie: corner 2
    assert vid[2, 2] == 0 and vid[2, 14] == 1 and vid[14, 8] == 2     # the corners themselves
    assert vid[3, 4] == 0 and vid[3, 12] == 1 and vid[12, 8] == 2     # and beside them
    assert (vid >= 0).sum() == (image > 0).sum() > 60
    assert set(np.unique(image)) == {0, 153}                          # trunc(255 * 1.5 / 2.5)
    # the premise: those four pixels ARE ties
    u, v, z = R.project(verts, TIE_K, TIE_LW, 1.0, 0.0, 0.0)
    A = R.setup(u, v, z, 16, 16, 1e-3)[0]
    for (x, y), tied in {(8, 6): (0, 1, 2), (8, 2): (0, 1), (11, 8): (1, 2), (5, 8): (0, 2)}.items():
        _, l0, l1, l2 = R.bary(u, v, A, float(x), float(y))
        a = [l0 / z[0], l1 / z[1], l2 / z[2]]
        assert len({a[i] for i in tied}) == 1 and max(a) == a[tied[0]], (x, y, a)


def test_vertex_ids_depth_range():
    verts, faces = tie_triangle()
    for zn, zf in ((2.5, 3.5), (1.0, 1.5)):                           # the triangle lies in front of / behind the range
        vid, image = PN.vertex_ids(verts, faces, TIE_K, TIE_LW, 16, 16, zn, zf)
        assert (vid == -1).all() and (image == 0).all()


# ---- the entry points --------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_exported_and_declared(lib):
    names = _lib.declared_symbols()
    for n in ("dfh_render_vertex_ids", "dfh_pool_features", "dfh_pool_features_workspace_bytes", "dfh_pool_features_tile"):
        assert n in names and n in _lib._SIGNATURES and hasattr(lib, n)
    assert lib.dfh_version() == 8 == _lib.ABI_VERSION


def _pool(lib, vid=PTR, feat=PTR, n_pixels=100, dim=16, n_verts=10, out=PTR, cnt=PTR, ws=PTR, ws_bytes=1 << 40):
    return lib.dfh_pool_features(vid, feat, n_pixels, dim, n_verts, out, cnt, ws, ws_bytes, None)


POOL_BAD = {
    "dim 0": dict(dim=0),
    "dim 65": dict(dim=65),
    "dim < 0": dict(dim=-1),
    "n_pixels < 0": dict(n_pixels=-1),
    "n_pixels 2^31": dict(n_pixels=2 ** 31),
    "n_verts < 0": dict(n_verts=-1),
    "n_verts 2^31": dict(n_verts=2 ** 31),
    "null vid": dict(vid=None),
    "null feat": dict(feat=None),
    "null feat_out": dict(out=None),
    "null cnt_out": dict(cnt=None),
    "null feat_out without pixels": dict(out=None, n_pixels=0),
    "null workspace": dict(ws=None),
    "misaligned workspace": dict(ws=PTR + 4),
    "workspace one byte short": "short",
    "workspace of 0 bytes": dict(ws_bytes=0),
}


@pytest.mark.parametrize("what", sorted(POOL_BAD))
@on_own_thread
def test_pool_refuses_bad_arguments_before_any_launch(lib, what):
    kw = POOL_BAD[what]
    if kw == "short":
        kw = dict(ws_bytes=lib.dfh_pool_features_workspace_bytes(100, 10) - 1)
    rc = _pool(lib, **kw)
    assert rc == BADARG, (what, rc)
    assert b"dfh_pool_features" in lib.dfh_last_error(), (what, lib.dfh_last_error())


@on_own_thread
def test_pool_size_queries(lib):
    f = lib.dfh_pool_features_workspace_bytes
    assert f(0, 10) == 0 and f(100, 0) == 0 and f(-1, 10) == 0 and f(100, -1) == 0 and f(2 ** 31, 10) == 0 and f(100, 2 ** 31) == 0
    assert f(100, 10) > 0 and f(100, 10) % 16 == 0
    assert f(100, 10) >= 2 * 4 * 100 + 4 * 10                         # the pixel list, the slots and the offsets at least
    sizes = [f(n, 1000) for n in (1, 255, 256, 257, 10 ** 4, 10 ** 6)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    tile = (ctypes.c_int * 4)()
    assert lib.dfh_pool_features_tile(tile) == OK and all(t > 0 for t in tile)
    assert lib.dfh_pool_features_tile(None) == BADARG and b"dfh_pool_features_tile" in lib.dfh_last_error()
    assert _pool(lib, n_verts=0, out=None, cnt=None, ws=None, ws_bytes=0) == OK      # no vertex: nothing to write, no launch


def _ids(lib, verts=PTR, n_verts=10, faces=PTR, n_faces=5, n_views=2, K=True, lw=True, H=8, W=8, center=True, znear=1e-3, ws=PTR,
         ws_bytes=1 << 40, zn=1.0, zf=3.5, vid=PTR, image=PTR):
    nk = max(1, min(n_views, 16))
    Ka = _lib.darr(np.tile(np.eye(3).reshape(-1), nk), 9 * nk) if K else None
    lwa = _lib.darr(np.tile(np.eye(4)[:3].reshape(-1), nk), 12 * nk) if lw else None
    ca = _lib.darr(np.zeros(3), 3) if center else None
    return lib.dfh_render_vertex_ids(verts, n_verts, faces, n_faces, n_views, Ka, lwa, H, W, 1.0, ca, 0.0, znear, ws, ws_bytes, zn, zf,
                                     vid, image, None)


IDS_BAD = {
    "null vid_out": dict(vid=None),
    "null workspace": dict(ws=None),
    "null verts": dict(verts=None),
    "null faces": dict(faces=None),
    "null K": dict(K=False),
    "null lw": dict(lw=False),
    "null center": dict(center=False),
    "workspace one byte short": "short",
    "no views": dict(n_views=0),
    "17 views": dict(n_views=17),
    "H 0": dict(H=0),
    "W 0": dict(W=0),
    "faces < 0": dict(n_faces=-1),
    "faces 2^31": dict(n_faces=2 ** 31),
    "verts < 0": dict(n_verts=-1),
    "znear 0": dict(znear=0.0),
    "zfar == znear": dict(zn=2.0, zf=2.0),
    "zfar < znear": dict(zn=3.5, zf=1.0),
    "znear nan": dict(zn=float("nan")),
    "zfar nan": dict(zf=float("nan")),
    "zfar inf": dict(zf=float("inf")),
    "znear -inf": dict(zn=float("-inf")),
}


@pytest.mark.parametrize("what", sorted(IDS_BAD))
@on_own_thread
def test_vertex_ids_refuses_bad_arguments_before_any_launch(lib, what):
    kw = IDS_BAD[what]
    if kw == "short":
        kw = dict(ws_bytes=lib.dfh_render_workspace_bytes(2, 8, 8, 5) - 1)
    rc = _ids(lib, **kw)
    assert rc == BADARG, (what, rc)
    assert b"dfh_render_vertex_ids" in lib.dfh_last_error(), (what, lib.dfh_last_error())


def test_python_layer_refuses_before_the_device():
    with pytest.raises(ValueError, match="faces"):
        descriptors.PooledDescriptors(lambda im: im)(np.zeros((4, 3)), None)
    with pytest.raises(ValueError, match="callable"):
        descriptors.PooledDescriptors(None)
    with pytest.raises(TypeError):
        descriptors.PooledDescriptors(lambda im: im, no_such_option=1)
