"""CPU: the numpy restatement of K17 (tests/color_np.py) against itself and against a voxel computed by hand, the share of voxels
the device comparisons leave out, the coloured OBJ file, and what dfh_integrate_color / dfh_sample_colors do with arguments they
cannot use.  Validation comes before any HIP call, so no GPU is needed: device pointers are dummy non-null integers."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from dynamicfusion_body_amd import _lib, build, mesh

import color_np as CN
import warped_np as WN

OK, BADARG = 0, -1
PTR = 0x1000
BIG = 1 << 30


@functools.lru_cache(maxsize=None)
def scene_of(name):
    if name == "skewed main":
        return WN.skewed_scene(scene_of("main"))
    return {"main": WN.main_scene, "ragged": WN.ragged_scene, "clustered": WN.clustered_scene}[name]()


@functools.lru_cache(maxsize=None)
def volumes(name, knn=4):
    """The restatement's canonical volumes after the scene's two views (float64), never written to."""
    T, Wt, _, _ = WN.restate(scene_of(name), knn)
    T.setflags(write=False)
    Wt.setflags(write=False)
    return T, Wt


# ---------------------------------------------------------------------------------------------- (a) the restatement against itself
def test_views_in_one_call_are_one_call_per_view():
    sc = scene_of("main")
    T, Wt = volumes("main")
    imgs = CN.color_images(sc)
    C, masks, _ = CN.restate(sc, 4, CN.pattern(sc["shape"]), T, Wt, imgs, 1.5, wmax=5.0)
    C2 = CN.pattern(sc["shape"])
    for v in range(2):
        one = dict(sc, depths=sc["depths"][v:v + 1], lws=sc["lws"][v:v + 1])
        CN.restate(one, 4, C2, T, Wt, imgs[v:v + 1], 1.5, wmax=5.0)
    assert masks[0].sum() > 100 and masks[1].sum() > 100 and (masks[0] & masks[1]).sum() > 20
    assert np.array_equal(C, C2)
    changed = np.any(C != CN.pattern(sc["shape"]), axis=-1)
    assert np.array_equal(changed, masks.any(axis=0))
    assert (C[..., 3] == 5.0).any()                                   # the cap is hit (the pattern starts at 1..4)


@pytest.mark.parametrize("knn", [1, 4, 8])
def test_no_nodes_is_the_identity_field(knn):
    sc = scene_of("main")
    T, Wt = volumes("main")
    imgs = CN.color_images(sc)
    C, masks, _ = CN.restate(sc, knn, CN.pattern(sc["shape"]), T, Wt, imgs, 2.0, warp=False)
    ident = dict(sc, node_dq=np.tile(WN.IDENT, (len(sc["node_pos"]), 1)), lw_dq=WN.IDENT)
    C2, masks2, _ = CN.restate(ident, knn, CN.pattern(sc["shape"]), T, Wt, imgs, 2.0)
    assert masks.any() and np.array_equal(masks, masks2) and np.array_equal(C, C2)


def hand_case():
    """A 4^3 grid seen through K = [[2,0,1],[0,2,1],[0,0,1]] with the identity extrinsic, scale 1, centre 0, tsdf_res 0 (so a
    voxel's world position is its index).  Voxel (1,2,2): K l = (4, 6, 2), (u, v) = (2, 3), depth -2.25 there, sd = 0.25.
    Voxel (1,2,3): K l = (5, 7, 3), (u, v) = (1.67, 2.33) -> pixel (2, 2), depth -3.5, sd = 0.5: outside band_sd = 0.3.
    Voxel (1,2,1): K l = (3, 5, 1), (u, v) = (3, 5): v is not < H - 1 = 5.  Voxel (2,2,2) would pass but has w = 0; (1,1,2) has
    |T| = 0.75 > band_vox."""
    K = np.array([[2.0, 0, 1], [0, 2, 1], [0, 0, 1]])
    depth = np.full((6, 6), -9.0, dtype=np.float32)
    depth[3, 2], depth[2, 2] = -2.25, -3.5
    img = np.zeros((6, 6, 4), dtype=np.uint8)
    img[3, 2] = (10, 20, 30, 99)
    img[2, 2] = (200, 200, 200, 0)
    T = np.full((4, 4, 4), 0.25)
    Wt = np.zeros((4, 4, 4))
    for i in ((1, 2, 2), (1, 2, 3), (1, 2, 1), (1, 1, 2)):
        Wt[i] = 1.0
    T[1, 1, 2] = 0.75
    C = np.zeros((4, 4, 4, 4), dtype=np.float32)
    C[...] = (100.0, 100.0, 100.0, 3.0)
    args = dict(depths=[depth], colors=[img], lws=[np.eye(4)[:3]], K=K, Kinv=np.linalg.inv(K), scale=1.0, center=np.zeros(3),
                tdist=1.0, band_vox=0.5, band_sd=0.3, tsdf_res=0)
    return C, T, Wt, args


def test_a_voxel_computed_by_hand():
    C, T, Wt, a = hand_case()
    C0 = C.copy()
    CN.integrate_color_np(C, T, Wt, a["depths"], a["colors"], a["lws"], a["K"], a["Kinv"], a["scale"], a["center"], a["tdist"],
                          a["band_vox"], a["band_sd"], tsdf_res=0)
    assert C[1, 2, 2].tolist() == [77.5, 80.0, 82.5, 4.0]              # (100 * 3 + pix) / 4
    C0[1, 2, 2] = C[1, 2, 2]
    assert np.array_equal(C, C0)                                       # nothing else moved
    # the cap: wmax = 3.5 leaves wc at 3.5
    C, T, Wt, a = hand_case()
    CN.integrate_color_np(C, T, Wt, a["depths"], a["colors"], a["lws"], a["K"], a["Kinv"], a["scale"], a["center"], a["tdist"],
                          a["band_vox"], a["band_sd"], wmax=3.5, tsdf_res=0)
    assert C[1, 2, 2].tolist() == [77.5, 80.0, 82.5, 3.5]


def test_sample_colors_by_hand():
    C = np.zeros((2, 2, 2, 4), dtype=np.float32)
    C[0, 0, 0] = (10, 20, 30, 1)
    C[1, 0, 0] = (30, 40, 50, 2)
    C[0, 1, 1] = (255, 255, 255, 0)                                   # never coloured: does not count
    pts = np.array([[0.25, 0.0, 0.0], [0.0, 1.0, 1.0], [1.0, 0.0, 0.0], [1.5, 0, 0], [np.nan, 0, 0], [0.5, 0.5, 0.5]])
    rgb, valid = CN.sample_colors_np(C, pts)
    assert valid.tolist() == [True, False, True, False, False, True]
    assert rgb[0].tolist() == [15.0, 25.0, 35.0] and rgb[2].tolist() == [30.0, 40.0, 50.0]
    assert rgb[5].tolist() == [20.0, 30.0, 40.0]                      # two coloured corners of equal weight
    assert not rgb[[1, 3, 4]].any()
    # a slab that holds only the upper x plane: the lower corner does not count
    rgb, valid = CN.sample_colors_np(C[1:], pts, res=(2, 2, 2), x_range=(1, 2))
    assert valid.tolist() == [True, False, True, False, False, True] and rgb[0].tolist() == [30.0, 40.0, 50.0]
    rgb, valid = CN.sample_colors_np(C[:1], pts, res=(2, 2, 2), x_range=(0, 1))
    assert valid.tolist() == [True, False, False, False, False, True] and rgb[0].tolist() == [10.0, 20.0, 30.0]


# ---------------------------------------------------------------------------------------------- (b) the exclusion cap
LIVE = {"main": (428, 622, 881), "ragged": (38, 57, 80), "clustered": (44, 73, 105), "skewed main": (431, 622, 884)}


@pytest.mark.parametrize("name", ["main", "ragged", "clustered", "skewed main"])
def test_scenes_stay_clear_of_the_decision_boundaries(name):
    sc = scene_of(name)
    T, Wt = volumes(name)
    imgs = CN.color_images(sc)
    for band, n_live in zip((1.0, 1.5, 2.0), LIVE[name]):
        live = (Wt > 0) & (np.abs(T) <= band)
        assert live.sum() == n_live
        C, masks, mg = CN.restate(sc, 4, CN.pattern(sc["shape"]), T, Wt, imgs, band)
        ex = CN.excluded(mg)
        print(name, band, "live", live.sum(), "coloured", masks.any(axis=0).sum(), "excluded", ex.sum())
        assert live.sum() > 0 and masks.any()
        assert not (ex & ~live).any()
        assert ex.sum() <= WN.MAX_EXCLUDED * live.sum()


def test_recovery_scene_matches_its_record():
    """tests/golden/color_recovery.json is color_np.recovery_record()'s output: the numpy chain (oracle fuse_depths, oracle
    marching cubes, the colour restatement) on the sphere painted with a smooth colour field.  The GPU test holds the device to the
    same numbers.  About 58 % of the level-0 vertices are invalid: two views from the front leave the far side of the truncation
    band facing unobserved voxels, and marching cubes closes the band there with a sheet no view coloured."""
    import json
    import os
    rec = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_recovery.json")))
    got = CN.recovery_record()
    print(got)
    assert got["n_vertices"] == rec["n_vertices"] > 500
    assert abs(got["rms"] - rec["rms"]) <= 1e-6 and abs(got["valid_share"] - rec["valid_share"]) <= 1e-6
    assert 0.0 < got["valid_share"] < 1.0


# ---------------------------------------------------------------------------------------------- (c) the OBJ file
def test_obj_round_trip_with_colours(tmp_path):
    rng = np.random.default_rng(1)
    verts, normals = rng.normal(size=(7, 3)), rng.normal(size=(7, 3))
    faces = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6]])
    rgb = rng.uniform(-20, 280, size=(7, 3))
    rgb[2] = (12.5, 13.5, 254.6)                                      # rint: half to even
    valid = np.ones(7, dtype=bool)
    valid[4] = False
    plain, colored = tmp_path / "plain.obj", tmp_path / "colored.obj"
    mesh.write_obj(str(plain), verts, faces, normals)
    mesh.write_obj(str(colored), verts, faces, normals, colors=rgb, valid=valid)
    want = "".join("v %f %f %f\n" % tuple(v) for v in verts) + "".join("vn %f %f %f\n" % tuple(n) for n in normals) + \
        "".join("f %d//%d %d//%d %d//%d\n" % (a + 1, a + 1, b + 1, b + 1, c + 1, c + 1) for a, b, c in faces)
    assert open(plain).read() == want                                 # byte for byte what it was
    assert mesh.read_obj_colors(str(plain)) is None
    got = mesh.read_obj_colors(str(colored))
    exp = np.clip(np.rint(rgb), 0, 255) / 255.0
    exp[4] = 0.5
    assert got.shape == (7, 3) and np.abs(got - exp).max() <= 5e-7    # "%f": six decimals
    assert np.abs(got[2] * 255 - (12, 14, 255)).max() < 1e-3
    for a, b in zip(mesh.read_obj(str(plain)), mesh.read_obj(str(colored))):
        assert np.array_equal(a, b)
    lines = open(colored).read().splitlines()
    assert len(lines[0].split()) == 7 and lines[7:] == open(plain).read().splitlines()[7:]
    with pytest.raises(ValueError):
        mesh.write_obj(str(colored), verts, faces, normals, colors=rgb[:3])


# ---------------------------------------------------------------------------------------------- (d) bad arguments
@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def on_own_thread(test):
    """dfh_last_error() is kept per thread: the refused calls are made on a thread of their own."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        with ThreadPoolExecutor(1) as ex:
            return ex.submit(test, *args, **kwargs).result()
    return run


def cvolume(rgbw=PTR, res=(8, 8, 16), x_range=None):
    return _lib.ColorVolume(rgbw, _lib.slab(res, x_range))


def volume(tsdf=PTR, tsdf_w=PTR, dtype=_lib.F32, res=(8, 8, 16), x_range=None):
    return _lib.Volume(tsdf, tsdf_w, dtype, _lib.slab(res, x_range))


_keep = []


def views(n=2, depth=PTR, null_map=None, dtype=_lib.F32, H=4, W=4, scale=0.05, lw=True, no_maps=False):
    ptrs = (ctypes.c_void_p * max(n, 1))(*[depth if i != null_map else 0 for i in range(max(n, 1))])
    lws = (ctypes.c_double * (12 * max(n, 1)))()
    _keep[:] = [ptrs, lws]
    v = _lib.DepthViews()
    v.n_views = n
    v.depth = None if no_maps else ctypes.cast(ptrs, ctypes.POINTER(ctypes.c_void_p))
    v.depth_dtype, v.H, v.W = dtype, H, W
    v.K = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    v.Kinv = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    v.lw = ctypes.cast(lws, ctypes.POINTER(ctypes.c_double)) if lw else None
    v.scale = scale
    v.tsdf_res = 8
    return v


def images(n=2, null_image=None):
    return (ctypes.c_void_p * n)(*[PTR if i != null_image else 0 for i in range(n)])


def nodes(pos=PTR, dq=PTR, w=PTR, n_nodes=16, knn=4):
    return _lib.Nodes(pos, dq, w, n_nodes, knn)


LW = (ctypes.c_double * 8)(1.0)
NAME = "dfh_integrate_color"


def call(lib, cvol="default", vol="default", vw="default", color="default", nd="default", lw_dq="default", band_vox=1.5,
         band_sd=0.1, wmax=100.0, workspace=PTR, nbytes=BIG, stored=0):
    cvol = cvolume() if cvol == "default" else cvol
    vol = volume() if vol == "default" else vol
    vw = views() if vw == "default" else vw
    color = images() if color == "default" else color
    nd = nodes() if nd == "default" else nd
    lw_dq = (LW if nd is not None else None) if lw_dq == "default" else lw_dq
    return lib.dfh_integrate_color(cvol, vol, vw, color, nd, lw_dq, 1.0, band_vox, band_sd, wmax, workspace, nbytes, stored, None)


BAD = {
    # dfh_integrate_depth_dqb's table
    "null volume": lambda: dict(vol=None),
    "null tsdf": lambda: dict(vol=volume(tsdf=0)),
    "null tsdf_w": lambda: dict(vol=volume(tsdf_w=0)),
    "volume dtype 2": lambda: dict(vol=volume(dtype=2)),
    "grid 0": lambda: dict(vol=volume(res=(8, 0, 16)), cvol=cvolume(res=(8, 0, 16))),
    "slab outside": lambda: dict(vol=volume(x_range=(4, 9)), cvol=cvolume(x_range=(4, 9))),
    "slab reversed": lambda: dict(vol=volume(x_range=(5, 4)), cvol=cvolume(x_range=(5, 4))),
    "null views": lambda: dict(vw=None),
    "null node_pos": lambda: dict(nd=nodes(pos=0)),
    "null node_dq": lambda: dict(nd=nodes(dq=0)),
    "null node_w": lambda: dict(nd=nodes(w=0)),
    "n_views -1": lambda: dict(vw=views(n=-1)),
    "n_views 17": lambda: dict(vw=views(n=17), color=images(17)),
    "null map table": lambda: dict(vw=views(no_maps=True)),
    "null lw table": lambda: dict(vw=views(lw=False)),
    "null map 1": lambda: dict(vw=views(null_map=1)),
    "H 1": lambda: dict(vw=views(H=1)),
    "W 1": lambda: dict(vw=views(W=1)),
    "depth dtype 2": lambda: dict(vw=views(dtype=2)),
    "depth dtype -1": lambda: dict(vw=views(dtype=-1)),
    "scale 0": lambda: dict(vw=views(scale=0.0)),
    "knn 0": lambda: dict(nd=nodes(knn=0)),
    "knn 9": lambda: dict(nd=nodes(knn=9)),
    "3 nodes, knn 4": lambda: dict(nd=nodes(n_nodes=3)),
    "null workspace": lambda: dict(workspace=0),
    # ... and the colour call's own
    "null cvol": lambda: dict(cvol=None),
    "null rgbw": lambda: dict(cvol=cvolume(rgbw=0)),
    "null color table": lambda: dict(color=None),
    "null image 1": lambda: dict(color=images(null_image=1)),
    "slab mismatch x": lambda: dict(cvol=cvolume(x_range=(0, 7))),
    "slab mismatch res": lambda: dict(cvol=cvolume(res=(8, 8, 8))),
    "band_vox 0": lambda: dict(band_vox=0.0),
    "band_vox -1": lambda: dict(band_vox=-1.0),
    "band_vox nan": lambda: dict(band_vox=float("nan")),
    "band_sd 0": lambda: dict(band_sd=0.0),
    "band_sd nan": lambda: dict(band_sd=float("nan")),
    "wmax 0.5": lambda: dict(wmax=0.5),
    "wmax nan": lambda: dict(wmax=float("nan")),
    "nodes without lw_dq": lambda: dict(lw_dq=None),
    "lw_dq without nodes": lambda: dict(nd=None, lw_dq=LW),
    "stored indices without nodes": lambda: dict(nd=None, stored=1),
}


@pytest.mark.parametrize("case", sorted(BAD))
@on_own_thread
def test_bad_arguments_are_refused(lib, case):
    rc = call(lib, **BAD[case]())
    assert rc == BADARG, (case, rc)
    assert NAME.encode() in lib.dfh_last_error(), (case, lib.dfh_last_error())


@on_own_thread
def test_workspace_sizes(lib):
    vol = volume()
    need = lib.dfh_dqb_workspace_bytes(ctypes.byref(vol.slab))
    assert need > 0
    assert call(lib, nbytes=need - 1) == BADARG
    assert NAME.encode() in lib.dfh_last_error() and str(need).encode() in lib.dfh_last_error()
    # stored indices from a buffer that has no index region
    cached = lib.dfh_dqb_workspace_bytes_cached(ctypes.byref(vol.slab), 4, 16, 1)
    assert cached > need
    assert call(lib, nbytes=need, stored=1) == BADARG and call(lib, nbytes=cached - 1, stored=1) == BADARG
    assert b"index region" in lib.dfh_last_error()


@on_own_thread
def test_nothing_to_do_is_ok_without_a_launch(lib):
    """An empty slab and a call without views return DFH_OK before any HIP call (this process has no device), with and without
    nodes and also without a workspace; their other arguments are still checked."""
    empty = dict(vol=volume(x_range=(3, 3)), cvol=cvolume(x_range=(3, 3)))
    assert call(lib, workspace=0, nbytes=0, **empty) == OK
    assert call(lib, nd=None, workspace=0, nbytes=0, **empty) == OK
    assert call(lib, vw=views(n=0), workspace=0, nbytes=0) == OK
    assert call(lib, vw=views(n=0, no_maps=True, lw=False), color=None, nd=None) == OK
    assert call(lib, band_vox=float("inf"), band_sd=float("inf"), wmax=1.0, **empty) == OK      # +inf bands, wmax 1: allowed
    assert call(lib, band_vox=0.0, **empty) == BADARG
    assert call(lib, vw=views(n=0), nd=nodes(knn=9)) == BADARG
    assert call(lib, vw=views(n=0, scale=0.0)) == BADARG
    assert call(lib, vw=views(n=0), cvol=cvolume(x_range=(0, 7))) == BADARG


@on_own_thread
def test_sample_colors_refuses_bad_arguments(lib):
    name = b"dfh_sample_colors"

    def refused(rc):
        assert rc == BADARG and name in lib.dfh_last_error(), (rc, lib.dfh_last_error())
    f = lib.dfh_sample_colors
    refused(f(None, PTR, 5, PTR, PTR, None))
    refused(f(cvolume(), PTR, -1, PTR, PTR, None))                     # a negative count
    refused(f(cvolume(), PTR, 1 << 31, PTR, PTR, None))
    refused(f(cvolume(), None, 5, None, None, None))                   # null pointers with a positive count
    refused(f(cvolume(), None, 5, PTR, PTR, None))
    refused(f(cvolume(), PTR, 5, None, PTR, None))
    refused(f(cvolume(), PTR, 5, PTR, None, None))
    refused(f(cvolume(rgbw=0), PTR, 5, PTR, PTR, None))
    refused(f(cvolume(res=(8, 0, 16)), PTR, 0, PTR, PTR, None))        # a bad slab, refused even with nothing to do
    refused(f(cvolume(x_range=(4, 9)), PTR, 0, PTR, PTR, None))
    assert f(cvolume(), None, 0, None, None, None) == OK               # a count of 0 with null pointers: nothing to do
    assert f(cvolume(rgbw=0), PTR, 0, PTR, PTR, None) == OK


def test_bindings_and_abi_version(lib):
    assert lib.dfh_version() == 8 == _lib.ABI_VERSION
    for name in ("dfh_integrate_color", "dfh_sample_colors"):
        assert name in _lib._SIGNATURES and name in _lib.declared_symbols()
    assert _lib.STRUCTS["dfh_color_volume"] is _lib.ColorVolume
