"""CPU: what dfh_integrate_depth_dqb (K1w: depth maps fused into the canonical volume through the warp field) does with arguments
it cannot use, what its Python wrappers refuse, and the identity anchor of its numpy restatement.  Validation comes before any
HIP call, so no GPU is needed: device pointers are dummy non-null integers that nothing dereferences."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from oracle import oracle_np as O
from dynamicfusion_body_amd import Fusion, _lib, build, kernels, scene

import warped_np as WN

OK, BADARG = 0, -1
PTR = 0x1000                                    # a "device pointer"
BIG = 1 << 30                                   # a workspace size that is always enough
NAME = "dfh_integrate_depth_dqb"


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


def nodes(pos=PTR, dq=PTR, w=PTR, n_nodes=16, knn=4):
    return _lib.Nodes(pos, dq, w, n_nodes, knn)


LW = (ctypes.c_double * 8)(1.0)


def call(lib, vol="default", vw="default", nd="default", lw_dq=LW, weight_mode=0, workspace=PTR, nbytes=BIG, rebuild=1):
    vol = volume() if vol == "default" else vol
    vw = views() if vw == "default" else vw
    nd = nodes() if nd == "default" else nd
    return lib.dfh_integrate_depth_dqb(vol, vw, nd, lw_dq, 1.0, 100.0, weight_mode, workspace, nbytes, rebuild, None)


BAD = {
    "null volume": lambda: dict(vol=None),
    "null tsdf": lambda: dict(vol=volume(tsdf=0)),
    "null tsdf_w": lambda: dict(vol=volume(tsdf_w=0)),
    "volume dtype 2": lambda: dict(vol=volume(dtype=2)),
    "grid 0": lambda: dict(vol=volume(res=(8, 0, 16))),
    "slab outside": lambda: dict(vol=volume(x_range=(4, 9))),
    "slab reversed": lambda: dict(vol=volume(x_range=(5, 4))),
    "null views": lambda: dict(vw=None),
    "null nodes": lambda: dict(nd=None),
    "null lw_dq": lambda: dict(lw_dq=None),
    "null node_pos": lambda: dict(nd=nodes(pos=0)),
    "null node_dq": lambda: dict(nd=nodes(dq=0)),
    "null node_w": lambda: dict(nd=nodes(w=0)),
    "n_views -1": lambda: dict(vw=views(n=-1)),
    "n_views 17": lambda: dict(vw=views(n=17)),
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
    "weight_mode 2": lambda: dict(weight_mode=2),
    "weight_mode -1": lambda: dict(weight_mode=-1),
    "null workspace": lambda: dict(workspace=0),
}


@pytest.mark.parametrize("case", sorted(BAD))
@on_own_thread
def test_bad_arguments_are_refused(lib, case):
    rc = call(lib, **BAD[case]())
    assert rc == BADARG, (case, rc)
    assert NAME.encode() in lib.dfh_last_error(), (case, lib.dfh_last_error())


@on_own_thread
def test_workspace_size_is_that_of_the_volume_fusion(lib):
    vol = volume()
    need = lib.dfh_dqb_workspace_bytes(ctypes.byref(vol.slab))
    assert need > 0
    assert call(lib, vol=vol, nbytes=need - 1) == BADARG
    assert NAME.encode() in lib.dfh_last_error() and str(need).encode() in lib.dfh_last_error()
    assert call(lib, vol=vol, nbytes=need - 1, rebuild=0) == BADARG


@on_own_thread
def test_nothing_to_do_is_ok_without_a_launch(lib):
    """An empty slab and a call without views return DFH_OK before any HIP call (this process has no device) -- also without a
    workspace; their other arguments are still checked."""
    assert call(lib, vol=volume(x_range=(3, 3)), workspace=0, nbytes=0) == OK
    assert call(lib, vw=views(n=0), workspace=0, nbytes=0) == OK
    assert call(lib, vw=views(n=0, no_maps=True, lw=False)) == OK
    assert call(lib, vol=volume(x_range=(3, 3)), weight_mode=5) == BADARG
    assert call(lib, vw=views(n=0), nd=nodes(knn=9)) == BADARG
    assert call(lib, vw=views(n=0, scale=0.0)) == BADARG


def test_the_abi_version_did_not_move(lib):
    assert lib.dfh_version() == 8 == _lib.ABI_VERSION
    assert NAME in _lib._SIGNATURES and NAME in _lib.declared_symbols()
    hdr = open(_lib.HEADER_PATH).read()
    assert "#define DFH_WARPED_W_UNIT 0" in hdr and "#define DFH_WARPED_W_NODE_DISTANCE 1" in hdr
    assert kernels.WARPED_WEIGHTS == {"unit": 0, "node_distance": 1}


# ---------------------------------------------------------------------------------------------- Python wrappers
def test_kernels_wrapper_refuses_before_it_needs_a_device():
    d = torch.zeros((4, 6), dtype=torch.float32)
    lw = np.eye(4)[:3]
    args = (np.eye(3), np.eye(3))
    tail = (1.0, np.zeros(3), 1.0, np.zeros((4, 3)), np.zeros((4, 8)), np.ones(4), 4, WN.IDENT)
    with pytest.raises(ValueError, match="length of camera matrix array"):
        kernels.integrate_depth_dqb(None, None, [d, d], *args, [lw], *tail)
    with pytest.raises(ValueError, match="weight must be one of"):
        kernels.integrate_depth_dqb(None, None, [d], *args, [lw], *tail, weight="mean")
    with pytest.raises(ValueError, match="same shape and dtype"):
        kernels.integrate_depth_dqb(None, None, [d, torch.zeros((4, 5))], *args, [lw, lw], *tail)
    with pytest.raises(ValueError, match="same shape and dtype"):
        kernels.integrate_depth_dqb(None, None, [d, d.double()], *args, [lw, lw], *tail)
    with pytest.raises(ValueError, match="2-D"):
        kernels.integrate_depth_dqb(None, None, [d[0]], *args, [lw], *tail)
    with pytest.raises(ValueError, match="2-D"):
        kernels.integrate_depth_dqb(None, None, [np.zeros((4, 6))], *args, [lw], *tail)


def test_fusion_wrapper_refuses_before_it_needs_a_device():
    f = Fusion(np.zeros((4, 4, 4)), 1.0)
    d, lw = np.zeros((4, 6)), np.eye(4)[:3]
    with pytest.raises(ValueError, match="needs the intrinsics"):
        f.updateTSDF_depths([d], [lw])
    f._K, f._Kinv = np.eye(3), np.eye(3)
    with pytest.raises(ValueError, match="length of camera matrix array"):
        f.updateTSDF_depths([d, d], [lw])
    with pytest.raises(ValueError, match="weight must be one of"):
        f.updateTSDF_depths([d], [lw], weight="mean")
    with pytest.raises(ValueError, match="3x4"):
        f.updateTSDF_depths([d], [np.eye(4)])
    with pytest.raises(ValueError, match="2-D"):
        f.updateTSDF_depths([d[0]], [lw])
    with pytest.raises(ValueError, match="same shape"):
        f.updateTSDF_depths([d, np.zeros((4, 5))], [lw, lw])


# ---------------------------------------------------------------------------------------------- the identity anchor
@pytest.mark.parametrize("knn", [1, 3, 4, 8])
def test_restatement_is_fuse_depths_under_the_identity_field(knn):
    """With every node DQ the identity the warped position of an integer voxel index is that index, exactly, and the restatement
    with unit weights reproduces oracle_np.fuse_depths bit for bit: what pins the device kernel to K1 with torch.equal."""
    sc = WN.main_scene()
    sc = dict(sc, node_dq=np.tile(WN.IDENT, (len(sc["node_pos"]), 1)), lw_dq=WN.IDENT)
    R = sc["shape"][0]
    g = np.stack(np.meshgrid(*[np.arange(R, dtype=np.float64)] * 3, indexing="ij"), axis=-1)
    loc = O.knn_bruteforce(g, sc["node_pos"], knn)
    q = O.warp(g, sc["node_dq"][loc], sc["node_pos"][loc], sc["node_w"][loc], m_lw=sc["lw_dq"])
    assert np.array_equal(q, g)
    T, Wt, masks, _ = WN.restate(sc, knn, "unit", wmax=100.0)
    To, Wo = WN.start_volumes(sc)
    for v in range(2):
        _, _, m = O.fuse_depths(sc["depths"][v], sc["lws"][v], sc["K"], sc["Kinv"], To, Wo, sc["tdist"], tsdf_res=R, scale=sc["scale"],
                                center=sc["center"], wmax=100.0, return_mask=True)
        assert np.array_equal(m, masks[v]) and m.sum() > 15000
    assert np.array_equal(T, To) and np.array_equal(Wt, Wo)


def test_scenes_stay_clear_of_the_decision_boundaries():
    """The exclusion rule leaves out well under 0.5 % of the voxels of every scene the GPU tests compare against the
    restatement, and the scenes exercise what they are for: most voxels update, the weight cap is hit."""
    for sc, knn in ((WN.main_scene(), 4), (WN.ragged_scene(), 3), (WN.clustered_scene(), 4)):
        for weight in ("unit", "node_distance"):
            T, Wt, masks, mg = WN.restate(sc, knn, weight, wmax=7.0 if weight == "node_distance" else 1.0)
            assert WN.excluded(mg).mean() <= WN.MAX_EXCLUDED
            assert masks[0].mean() > 0.4 and masks[1].mean() > 0.4
            assert (Wt == (7.0 if weight == "node_distance" else 1.0)).sum() > 0.3 * T.size
