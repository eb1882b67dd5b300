"""GPU: the depth preprocessing kernel (kernels.depth_prep, dfh_depth_prep) against its numpy restatement
(tests/depth_prep_np.py), bit for bit on both outputs, and its hooks in FusionDM and SlabFrame against the same calls on
pre-cleaned maps."""
import functools

import numpy as np
import pytest
import torch

import depth_prep_cases as C
import depth_prep_np as DN
from dynamicfusion_body_amd import FusionDM, _lib, kernels, scene
from dynamicfusion_body_amd.depth_prep import DepthPrep
from dynamicfusion_body_amd.pipeline import SlabFrame

pytestmark = pytest.mark.gpu

RADII = (0, 1, 2, 3, 8)
FIXED_SHAPES = {"2x2": (2, 2), "3x3": (3, 3), "5x7": (5, 7), "scene 37x53": (37, 53), "scene 19x70": (19, 70)}
TILE_SHAPES = {"tile": (0, 0, 1), "tile +1 -1": (1, -1, 1), "tile -1 +1": (-1, 1, 1), "2 tiles + 1": (1, 1, 2)}   # (dh, dw, factor)


def shape_of(name):
    if name in FIXED_SHAPES:
        return FIXED_SHAPES[name]
    th, tw = kernels.depth_prep_tile()
    dh, dw, k = TILE_SHAPES[name]
    return k * th + dh, k * tw + dw


def depth_map(H, W, seed=1234, angle=20.0, dtype="float32"):
    return C.scene_map(H, W, angle=angle, seed=seed, dtype=dtype, bad=H >= 12 and W >= 12)


@functools.lru_cache(maxsize=None)
def reference(shape, radius, dtype="float32", views=1, mask=True, jump=C.SCENE_JUMP, cos=C.SCENE_COS):
    """(maps, clean, normals) of the restatement for `views` distinct maps of one shape; computed once, read-only."""
    maps = view_maps(shape, dtype, views)
    sp, lut, s = C.tables_np(radius)
    clean, nrm = DN.depth_prep(maps, C.scene_kinv(), radius, sp, lut, s, jump, cos, mask=mask)
    clean.setflags(write=False)
    nrm.setflags(write=False)
    return maps, clean, nrm


def view_maps(shape, dtype, views):
    H, W = shape
    maps = [depth_map(H, W, seed=1234 + 7 * v, angle=20.0 + 9.0 * v, dtype=dtype) for v in range(views)]
    if views >= 3:
        maps[1] = np.zeros((H, W), dtype=dtype)                                # a view without a single measurement
    return maps


def dev_tables(tables):
    sp, lut, s = tables
    return torch.from_numpy(np.ascontiguousarray(sp)).cuda(), torch.from_numpy(np.ascontiguousarray(lut)).cuda(), s


def run(maps, radius, tables=None, jump=C.SCENE_JUMP, cos=C.SCENE_COS, Kinv=None, **kw):
    tab = dev_tables(C.tables_np(radius) if tables is None else tables)
    dev = [torch.from_numpy(np.array(m)).cuda() for m in maps]
    clean, nrm = kernels.depth_prep(dev, C.scene_kinv() if Kinv is None else Kinv, tab, jump, cos, **kw)
    torch.cuda.synchronize()
    for m, d in zip(maps, dev):                                                # the inputs are only read
        assert np.array_equal(d.cpu().numpy(), m, equal_nan=True)
    return (None if clean is None else clean.cpu().numpy()), (None if nrm is None else nrm.cpu().numpy())


def same(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.isfinite(got).all()
    assert np.array_equal(got, want), "%d of %d values differ" % (int((got != want).sum()), got.size)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", list(FIXED_SHAPES) + list(TILE_SHAPES))
def test_shapes_and_radii(name, radius):
    shape = shape_of(name)
    maps, clean, nrm = reference(shape, radius)
    got_c, got_n = run(maps, radius)
    same(got_c, clean)
    same(got_n, nrm)
    if min(shape) >= 12:
        assert (got_c != 0).sum() >= 10 and (got_n != 0).any()


@pytest.mark.parametrize("name,radius", [("5x7", 1), ("scene 19x70", 3), ("tile -1 +1", 0), ("2 tiles + 1", 8)])
def test_relaid_normal_stores(name, radius):
    """Option k12_store = 1: the normals leave through LDS in runs of consecutive dwords instead of three strided stores per
    lane (the default) -- the same bits, ragged right and bottom tiles included; clean alone and normals alone as well."""
    maps, clean, nrm = reference(shape_of(name), radius)
    _lib.set_option("k12_store", 1)
    got_c, got_n = run(maps, radius)
    same(got_c, clean)
    same(got_n, nrm)
    same(run(maps, radius, want_normals=False)[0], clean)
    buf = torch.full(nrm.shape, 7.0, dtype=torch.float32, device="cuda")
    same(run(maps, radius, out=(None, buf))[1], nrm)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("views", [1, 3, 16])
def test_views_and_dtypes(views, dtype):
    maps, clean, nrm = reference((37, 53), 2, dtype=dtype, views=views)
    if dtype == "float64":
        assert maps[0].dtype == np.float64 and maps[0][1, 2] == -1e-50
        assert not np.array_equal(maps[0].astype(np.float32).astype(np.float64), maps[0])
    got_c, got_n = run(maps, 2)
    same(got_c, clean)
    same(got_n, nrm)
    for v in range(views):
        if views >= 3 and v == 1:
            assert not got_c[v].any() and not got_n[v].any()
        else:
            assert (got_c[v] != 0).sum() >= 10
            assert all(not np.array_equal(got_c[v], got_c[u]) for u in range(v))
    if dtype == "float64":
        assert got_c[0][1, 2] == 0                                             # -1e-50 rounds to -0.0: no measurement


@pytest.mark.parametrize("mask", [False, True])
def test_mask_and_missing_outputs(mask):
    maps, clean, nrm = reference((19, 70), 3, views=3, mask=mask)
    got_c, got_n = run(maps, 3, mask=mask)
    same(got_c, clean)
    same(got_n, nrm)
    if not mask:
        masked = reference((19, 70), 3, views=3, mask=True)[1]
        assert ((got_c != 0) & (masked == 0)).sum() >= 10                      # what the mask removes
    only_c, none_n = run(maps, 3, mask=mask, want_normals=False)
    assert none_n is None
    same(only_c, clean)
    V, (H, W) = len(maps), maps[0].shape
    buf = torch.full((V, H, W, 3), 7.0, dtype=torch.float32, device="cuda")
    none_c, only_n = run(maps, 3, mask=mask, out=(None, buf))
    assert none_c is None
    same(only_n, nrm)


@pytest.mark.parametrize("which,radius", [("sparse", 0), ("sparse", 1), ("sparse", 2), ("dense", 0), ("dense", 2)])
def test_exact_ties(which, radius):
    d, _ = C.tie_map() if which == "sparse" else C.tie_map_dense()
    tab = C.tie_tables(radius)
    want_c, want_n = DN.depth_prep([d], np.eye(3), radius, *tab, C.TIE_JUMP, 0.0, mask=False)
    got_c, got_n = run([d], radius, tables=tab, jump=C.TIE_JUMP, cos=0.0, Kinv=np.eye(3), mask=False)
    same(got_c, want_c)
    same(got_n, want_n)
    if which == "dense" and radius == 0:
        assert (got_n != 0).any(-1).sum() >= 10


def test_repeatable_and_stream_independent():
    maps, clean, nrm = reference((37, 53), 3, views=3)
    a = run(maps, 3)
    b = run(maps, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run(maps, 3)
    same(c[0], clean)
    same(c[1], nrm)


def test_out_buffers_are_versioned():
    maps, clean, nrm = reference((37, 53), 2, views=3)
    V, (H, W) = len(maps), maps[0].shape
    out = (torch.zeros((V, H, W), dtype=torch.float32, device="cuda"), torch.zeros((V, H, W, 3), dtype=torch.float32, device="cuda"))
    v0 = (out[0]._version, out[1]._version)
    view = out[0][1]
    got_c, got_n = run(maps, 2, out=out)
    same(got_c, clean)
    same(got_n, nrm)
    assert out[0]._version > v0[0] and out[1]._version > v0[1] and view._version > v0[0]
    v1 = (out[0]._version, out[1]._version)
    run(maps, 2, out=out)
    assert out[0]._version > v1[0] and out[1]._version > v1[1]
    with pytest.raises(ValueError):
        run(maps, 2, out=(out[0][:2], out[1]))
    with pytest.raises(ValueError, match="dfh_depth_prep"):                    # in place: refused by the library, nothing launched
        kernels.depth_prep([out[0][v] for v in range(V)], C.scene_kinv(), dev_tables(C.tables_np(2)), 0.1, 0.5, out=(out[0], None))


# ---- the hooks: a DepthPrep inside the loop equals the loop on pre-cleaned maps ------------------------------------------------
R, N = 64, 64
H, W = 37, 53
ANGLES = (0.0, 40.0)
ANGLES4 = (0.0, 40.0, -40.0, 20.0)            # four views: from there on the solve culls views by the table's per-cell depth ranges


def prep():
    return DepthPrep(radius=2, sigma_s=1.5, sigma_r=0.05, max_jump=C.SCENE_JUMP, min_cos=0.5)


def make_frames(angles, blank=None):
    """Frame 0 builds the canonical volume, frames 1 and 2 follow the moving sphere.  blank = (frame, columns): that frame's maps
    carry no measurement in their first `columns` columns."""
    K = C.small_camera()
    scale = scene.grid_params(R)[0]
    lws = [scene.view_extrinsic(a) for a in angles]
    out = []
    for f in range(3):                                                         # frame 0 builds the canonical volume
        off = np.array([0.4, -0.25, 0.15]) * np.sin(0.5 * f) * scale
        out.append([torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.02, seed=11 + f,
                                                        sphere_offset=off)).cuda() for lw in lws])
    if blank is not None:
        for d in out[blank[0]]:
            d[:, :blank[1]] = 0
    return K, lws, out


@pytest.fixture(scope="module")
def frames():
    return make_frames(ANGLES)


def new_loop(K, lws, first, depth_prep=None):
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=2.0, distributed=False,
                   depth_prep=depth_prep)
    for d, lw in zip(first, lws):
        sf.integrate(d, lw)
    assert sf.refresh_samples() > 100
    return sf


def state(sf):
    torch.cuda.synchronize()
    return sf.T.clone(), sf.Wt.clone(), sf.fs.solver.node_dq.clone()


def equal_states(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("update", ["volume", "depth"])
def test_slab_frame_cleans_its_frame_once(frames, update):
    K, lws, fr = frames
    p = prep()
    a, b, raw = new_loop(K, lws, fr[0], depth_prep=p), new_loop(K, lws, fr[0]), new_loop(K, lws, fr[0])
    for ds in fr[1:]:
        na = a.step(ds, lws, gn_iters=3, update=update)
        cleaned, normals = p(ds, np.linalg.inv(K))
        nb = b.step(cleaned, lws, gn_iters=3, update=update)
        raw.step(ds, lws, gn_iters=3, update=update)
        assert na == nb > 100
        assert all(torch.equal(x, y) for x, y in zip(a.clean_depth, cleaned)) and torch.equal(a.live_normals, normals)
        assert tuple(a.live_normals.shape) == (len(ds), H, W, 3) and a.clean_depth[1].is_contiguous()
    sa, sb = state(a), state(b)
    assert equal_states(sa, sb)
    assert not equal_states(sa, state(raw))                                    # (the stage does change what the frame sees)
    assert raw.clean_depth is None and raw.live_normals is None


def test_reused_out_buffers_do_not_leave_a_stale_views_table():
    """The solver caches its packed views table on the maps' (data_ptr, _version): a second frame written into the SAME buffers
    must not be solved against the first frame's table.  That table holds, per view, the depth range of every 16 x 16-pixel
    cell, by which the solve drops views: the first frame's maps are blank in their first 32 columns, so a stale table would
    drop every view for the samples that the second frame does see there."""
    K, lws, fr = make_frames(ANGLES4, blank=(1, 32))
    p = prep()
    Kinv = np.linalg.inv(K)
    a, b = new_loop(K, lws, fr[0]), new_loop(K, lws, fr[0])
    out = (torch.empty((4, H, W), dtype=torch.float32, device="cuda"), torch.empty((4, H, W, 3), dtype=torch.float32, device="cuda"))
    ptr = out[0].data_ptr()
    for ds in fr[1:]:
        reused, _ = p(ds, Kinv, out=out)
        assert reused[0].data_ptr() == ptr
        a.step(reused, lws, gn_iters=3)
        fresh, _ = p(ds, Kinv)
        b.step(fresh, lws, gn_iters=3)
    assert equal_states(state(a), state(b))
    assert not torch.equal(p(fr[1], Kinv)[0][0], p(fr[2], Kinv)[0][0])          # (the two frames do differ)


def test_compute_live_tsdf_cleans_its_list():
    K = C.small_camera()
    lws = [scene.view_extrinsic(a) for a in ANGLES]
    maps = [scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.02) for lw in lws]
    p = prep()
    f = FusionDM(0.1, K, tsdf_res=R)
    assert f.depth_prep is None
    raw = [t.clone() for t in f.compute_live_tsdf(maps, lws, UseAutoAlignment=True, as_numpy=False)]
    f.depth_prep = p
    T, Wt = (t.clone() for t in f.compute_live_tsdf(maps, lws, UseAutoAlignment=True, as_numpy=False))
    g = FusionDM(0.1, K, tsdf_res=R)
    cleaned = p([torch.from_numpy(m).cuda() for m in maps], np.linalg.inv(K))[0]
    T2, W2 = g.compute_live_tsdf(cleaned, lws, UseAutoAlignment=True, as_numpy=False)
    assert torch.equal(T, T2) and torch.equal(Wt, W2)
    assert bool((Wt != 0).any()) and not torch.equal(Wt, raw[1])
