"""GPU: K1w (dfh_integrate_depth_dqb = depth maps fused into the canonical volume through the warp field) through
kernels.integrate_depth_dqb, against K1 under the identity field (bit for bit on float64 volumes), against its numpy restatement
(tests/warped_np.py) under a non-rigid field, and against itself across views, workspaces and slabs.

Bars.  float64 volumes: the changed-voxel mask is the restatement's, |dT| and |dw| <= 1e-12 (exp() of the blend weights
differs in the last ulp between libm and the device library: the bar of test_gpu_fuse_volume.py::test_dqb_vs_oracle).  float32
volumes: the same mask, w within one float32 rounding, |dT| <= 2 n eps32 (1 + |T|) with n views.  Voxels
whose decision hangs on that last ulp are left out by warped_np.excluded(), and every test asserts that they are fewer than 0.5 %."""
import functools

import numpy as np
import pytest
import torch

from dynamicfusion_body_amd import kernels

import warped_np as WN

pytestmark = pytest.mark.gpu

F32_EPS = float(np.finfo(np.float32).eps)
TORCH = {np.float64: torch.float64, np.float32: torch.float32}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to("cuda", dtype=dtype or t.dtype)


@functools.lru_cache(maxsize=None)
def scene_of(name):
    if name == "skewed ragged":
        return WN.skewed_scene(scene_of("ragged"))
    return {"main": WN.main_scene, "ragged": WN.ragged_scene, "clustered": WN.clustered_scene}[name]()


@functools.lru_cache(maxsize=None)
def reference(name, knn, weight, wmax, dtype):
    """The restatement's result, computed once per case and never written to."""
    T, Wt, masks, mg = WN.restate(scene_of(name), knn, weight, wmax, dtype)
    for a in (T, Wt, masks):
        a.setflags(write=False)
    return T, Wt, masks, WN.excluded(mg)


def run(sc, knn, weight="unit", wmax=100.0, dtype=np.float64, depths=None, lws=None, K=None, Kinv=None, node_dq=None, lw_dq=None,
        T=None, Wt=None, depth_dtype=None, **kw):
    """One integrate_depth_dqb call on fresh volumes (or on T / Wt): the volumes as device tensors."""
    if T is None:
        T0, W0 = WN.start_volumes(sc, dtype)
        T, Wt = dev(T0), dev(W0)
    depths = sc["depths"] if depths is None else depths
    depths = [d if isinstance(d, torch.Tensor) else dev(d, depth_dtype) for d in depths]
    kernels.integrate_depth_dqb(T, Wt, depths, sc["K"] if K is None else K, sc["Kinv"] if Kinv is None else Kinv,
                                sc["lws"] if lws is None else lws, sc["scale"], sc["center"], sc["tdist"], sc["node_pos"],
                                sc["node_dq"] if node_dq is None else node_dq, sc["node_w"], knn, sc["lw_dq"] if lw_dq is None else lw_dq,
                                wmax=wmax, weight=weight, tsdf_res=sc["tsdf_res"], **kw)
    return T, Wt


def compare(T, Wt, ref, sc, dtype, n_views=2):
    """The device volumes against a restatement's (T, Wt, masks, excluded)."""
    To, Wo, masks, ex = ref
    assert ex.mean() <= WN.MAX_EXCLUDED
    keep = ~ex
    Tn, Wn = T.cpu().numpy(), Wt.cpu().numpy()
    T0, W0 = WN.start_volumes(sc, dtype)
    changed = (Tn != T0) | (Wn != W0)
    upd = masks.any(axis=0)
    dT = np.abs(Tn.astype(np.float64) - To.astype(np.float64))[keep]
    dW = np.abs(Wn.astype(np.float64) - Wo.astype(np.float64))[keep]
    print("updated %d of %d, excluded %d, mask mismatches outside the exclusions %d, max |dT| %.3g, max |dw| %.3g"
          % (upd.sum(), upd.size, ex.sum(), (changed != upd)[keep].sum(), dT.max(), dW.max()))
    assert upd.any() and (~upd).any()
    assert np.array_equal(changed[keep], upd[keep])
    if dtype == np.float64:
        assert dT.max() <= 1e-12 and dW.max() <= 1e-12
    else:
        assert np.all(dW <= F32_EPS * np.abs(Wo.astype(np.float64))[keep])
        assert np.all(dT <= 2.0 * n_views * F32_EPS * (1.0 + np.abs(To.astype(np.float64))[keep]))


# ---------------------------------------------------------------------------------------------- 1. identity field = K1
@pytest.mark.parametrize("blend", ["identity", "zero"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("knn", [1, 3, 4, 8])
def test_identity_field_is_k1(knn, dtype, blend):
    """Every node DQ the identity (or zero: |b|_8 == 0, the identity blend), lw_dq the identity, unit weights: the warped
    position of a voxel is its index, exactly, and the call is K1 view after view."""
    sc = scene_of("main")
    N = len(sc["node_pos"])
    dq = np.tile(WN.IDENT, (N, 1)) if blend == "identity" else np.zeros((N, 8))
    T, Wt = run(sc, knn, "unit", 100.0, dtype, node_dq=dq, lw_dq=WN.IDENT)
    T0, W0 = WN.start_volumes(sc, dtype)
    Tk, Wk = dev(T0), dev(W0)
    for d, lw in zip(sc["depths"], sc["lws"]):
        kernels.integrate_depth(Tk, Wk, dev(d), sc["K"], sc["Kinv"], lw, sc["scale"], sc["center"], sc["tdist"], tsdf_res=sc["tsdf_res"])
    assert (Wk == 2).sum() > 5000 and (Wk == 0).sum() > 1000
    assert torch.equal(Wt, Wk)
    if dtype == np.float64:
        assert torch.equal(T, Tk)
    else:
        Tn, Tr = T.cpu().numpy().astype(np.float64), Tk.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(Tn - Tr) <= 2.0 * 2 * F32_EPS * (1.0 + np.abs(Tr)))


# ---------------------------------------------------------------------------------------------- 2. non-rigid field = restatement
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("weight,wmax", [("unit", 7.0), ("unit", 1.5), ("node_distance", 7.0)])
@pytest.mark.parametrize("knn", [1, 3, 4, 8])
def test_nonrigid_field_is_the_restatement(knn, weight, wmax, dtype):
    sc = scene_of("main")
    ref = reference("main", knn, weight, wmax, dtype)
    if weight == "node_distance" or wmax < 2:
        assert (ref[1] == wmax).sum() > 10000                      # the cap is hit
    T, Wt = run(sc, knn, weight, wmax, dtype)
    compare(T, Wt, ref, sc, dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("weight", ["unit", "node_distance"])
@pytest.mark.parametrize("name,knn", [("ragged", 3), ("clustered", 4)])
def test_ragged_grid_and_brute_force_fallback(name, knn, weight, dtype):
    """(13, 11, 21) voxels of a 21-grid: no extent is a multiple of the 4 x 4 x 16 brick.  320 nodes round one brick: more
    than the 256 candidates a brick keeps, so its voxels scan every node."""
    sc = scene_of(name)
    T, Wt = run(sc, knn, weight, 7.0, dtype)
    compare(T, Wt, reference(name, knn, weight, 7.0, dtype), sc, dtype)
    # ... and the stored-index mode on the same grid (its threads run along z, with a ragged last block)
    ws = kernels.dqb_workspace(sc["shape"], knn=knn, n_nodes=len(sc["node_pos"]), level=1)
    run(sc, knn, weight, 7.0, dtype, workspace=ws, rebuild_candidates=True)
    T2, W2 = run(sc, knn, weight, 7.0, dtype, workspace=ws, rebuild_candidates=False)
    assert torch.equal(T2, T) and torch.equal(W2, Wt)


# ---------------------------------------------------------------------------------------------- 3. views
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("weight", ["unit", "node_distance"])
def test_two_views_in_one_call_are_two_calls(weight, dtype):
    sc = scene_of("main")
    T, Wt = run(sc, 4, weight, 7.0, dtype)
    T2, W2 = run(sc, 4, weight, 7.0, dtype, depths=sc["depths"][:1], lws=sc["lws"][:1])
    run(sc, 4, weight, 7.0, dtype, depths=sc["depths"][1:], lws=sc["lws"][1:], T=T2, Wt=W2)
    assert (Wt != 0).sum() > 15000
    assert torch.equal(T, T2) and torch.equal(Wt, W2)


def test_more_than_sixteen_views_go_sixteen_at_a_time():
    sc = scene_of("ragged")
    depths, lws = [dev(d) for d in sc["depths"]] * 9, sc["lws"] * 9           # 18 views
    T, Wt = run(sc, 3, "node_distance", 50.0, np.float32, depths=depths, lws=lws)
    T2, W2 = run(sc, 3, "node_distance", 50.0, np.float32, depths=depths[:16], lws=lws[:16])
    run(sc, 3, "node_distance", 50.0, np.float32, depths=depths[16:], lws=lws[16:], T=T2, Wt=W2)
    assert torch.equal(T, T2) and torch.equal(Wt, W2) and (Wt == 50).any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_float64_maps_that_are_float32_exact(dtype):
    sc = scene_of("main")
    assert all(d.dtype == np.float32 for d in sc["depths"])
    T, Wt = run(sc, 4, "node_distance", 7.0, dtype)
    T2, W2 = run(sc, 4, "node_distance", 7.0, dtype, depth_dtype=torch.float64)
    assert torch.equal(T, T2) and torch.equal(Wt, W2)


@functools.lru_cache(maxsize=None)
def bad_depth_case(dtype, huge=False):
    """Pixels equal to 0, -inf and NaN under the sphere's footprint, in stripes.  huge: float64 maps with -1e306 in place of -inf:
    z * u overflows right of column 179 (no update, as for -inf) and stays finite left of it (an update by tdist)."""
    sc = scene_of("main")
    depths = [d.astype(np.float64) if huge else d.copy() for d in sc["depths"]]
    for d in depths:
        d[100:140:3, 120:200] = 0.0
        d[101:140:3, 120:200] = -1e306 if huge else -np.inf
        d[102:140:3, 120:200] = np.nan
    T, Wt, masks, mg = WN.restate(sc, 4, "node_distance", 7.0, dtype, depths=depths)
    plain = reference("main", 4, "node_distance", 7.0, dtype)
    assert (plain[2][0] & ~masks[0]).sum() > 200 and (plain[2][1] & ~masks[1]).sum() > 200      # the bad pixels lie under voxels that would update
    return depths, (T, Wt, masks, WN.excluded(mg))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bad_depth_values_update_nothing(dtype):
    sc = scene_of("main")
    depths, ref = bad_depth_case(dtype)
    T, Wt = run(sc, 4, "node_distance", 7.0, dtype, depths=depths)
    assert bool(torch.isfinite(T).all()) and bool(torch.isfinite(Wt).all())
    compare(T, Wt, ref, sc, dtype)
    # float64 maps: -inf and NaN travel unchanged
    T2, W2 = run(sc, 4, "node_distance", 7.0, dtype, depths=depths, depth_dtype=torch.float64)
    assert torch.equal(T2, T) and torch.equal(W2, Wt)
    # ... and a finite depth whose z * u overflows updates nothing either, while the same depth left of it does
    depths, ref = bad_depth_case(dtype, True)
    assert (ref[2] != bad_depth_case(dtype)[1][2]).sum() > 50
    T3, W3 = run(sc, 4, "node_distance", 7.0, dtype, depths=depths)
    compare(T3, W3, ref, sc, dtype)


@functools.lru_cache(maxsize=None)
def general_k_case(dtype):
    sc = scene_of("main")
    K, Kinv = WN.skewed(sc["K"])
    T, Wt, masks, mg = WN.restate(sc, 4, "node_distance", 7.0, dtype, K=K, Kinv=Kinv)
    return K, Kinv, (T, Wt, masks, WN.excluded(mg))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_general_intrinsics(dtype):
    sc = scene_of("main")
    K, Kinv, ref = general_k_case(dtype)
    assert Kinv[2, 0] != 0 and Kinv[2, 1] != 0
    T, Wt = run(sc, 4, "node_distance", 7.0, dtype, K=K, Kinv=Kinv)
    compare(T, Wt, ref, sc, dtype)


# ---------------------------------------------------------------------------------------------- 4. workspace
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("knn,name", [pytest.param(3, "main", id="3"), pytest.param(4, "main", id="4"), pytest.param(8, "main", id="8"),
                                      pytest.param(3, "skewed ragged", id="3-skewed ragged"),
                                      pytest.param(8, "skewed ragged", id="8-skewed ragged")])
def test_search_store_and_load_agree(knn, name, dtype):
    """skewed ragged: the general projection chain through the storing and the loading mode, on bricks and z-runs with ragged ends."""
    sc = scene_of(name)
    N = len(sc["node_pos"])
    base = kernels.dqb_workspace(sc["shape"])
    T, Wt = run(sc, knn, "node_distance", 7.0, dtype, workspace=base, rebuild_candidates=True)              # search only
    T1, W1 = run(sc, knn, "node_distance", 7.0, dtype, workspace=base, rebuild_candidates=False)            # ... of existing lists
    assert torch.equal(T1, T) and torch.equal(W1, Wt) and bool((Wt != 0).any()) and bool((Wt == 0).any())
    other_dq = WN.field(np.random.default_rng(3), N, 0.05, 0.2, 0.0)
    for level in (1, 2):
        ws = kernels.dqb_workspace(sc["shape"], knn=knn, n_nodes=N, level=level)
        assert ws.numel() > base.numel()
        T2, W2 = run(sc, knn, "node_distance", 7.0, dtype, workspace=ws, rebuild_candidates=True)           # search + store
        T3, W3 = run(sc, knn, "node_distance", 7.0, dtype, workspace=ws, rebuild_candidates=False)          # load
        assert torch.equal(T2, T) and torch.equal(W2, Wt) and torch.equal(T3, T) and torch.equal(W3, Wt)
        # the stored neighbourhoods do not depend on the node DQs: stored under another field, loaded under this one
        run(sc, knn, "node_distance", 7.0, dtype, node_dq=other_dq, workspace=ws, rebuild_candidates=True)
        T4, W4 = run(sc, knn, "node_distance", 7.0, dtype, workspace=ws, rebuild_candidates=False)
        assert torch.equal(T4, T) and torch.equal(W4, Wt)


def sphere_live(sc):
    shape = sc["shape"]
    g = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), axis=-1)
    tv = sc["tdist"] / sc["scale"]
    return np.clip(np.linalg.norm(g - (np.array(shape) / 2.0 + 0.4), axis=-1) - min(shape) / 3.1, -tv, tv)


def k3(sc, knn, dtype, workspace, rebuild, node_pos=None):
    T0, W0 = WN.start_volumes(sc, dtype)
    T, Wt = dev(T0), dev(W0)
    kernels.fuse_volume_dqb(T, Wt, dev(sphere_live(sc), torch.float32), sc["node_pos"] if node_pos is None else node_pos, sc["node_dq"],
                            sc["node_w"], knn, sc["lw_dq"], sc["tdist"] / sc["scale"], 7.0, workspace=workspace, rebuild_candidates=rebuild)
    return T, Wt


@pytest.mark.parametrize("dtype,knn", [(np.float32, 4), (np.float64, 3)])
def test_one_workspace_serves_the_volume_fusion_too(dtype, knn):
    """float32 volumes with knn 4 are fuse_volume_dqb's fast path and its cache format; float64 with knn 3 its exact kernel."""
    sc = scene_of("main")
    N = len(sc["node_pos"])
    T, Wt = run(sc, knn, "node_distance", 7.0, dtype)
    # indices stored by fuse_volume_dqb, loaded here
    ws = kernels.dqb_workspace(sc["shape"], knn=knn, n_nodes=N, level=2)
    k3(sc, knn, dtype, ws, True)
    T1, W1 = run(sc, knn, "node_distance", 7.0, dtype, workspace=ws, rebuild_candidates=False)
    assert torch.equal(T1, T) and torch.equal(W1, Wt)
    # ... which leaves that buffer's stored weights alone: the next fuse_volume_dqb call without a rebuild gives a fresh call's bits
    Tf, Wf = k3(sc, knn, dtype, kernels.dqb_workspace(sc["shape"]), True)
    assert (Wf != 0).sum() > 1000
    Tk, Wk = k3(sc, knn, dtype, ws, False)
    assert torch.equal(Tk, Tf) and torch.equal(Wk, Wf)
    # the converse: indices stored here -- over what fuse_volume_dqb stored for ANOTHER graph, weights included -- loaded there
    for level in (1, 2):
        ws = kernels.dqb_workspace(sc["shape"], knn=knn, n_nodes=N, level=level)
        k3(sc, knn, dtype, ws, True, node_pos=sc["node_pos"][::-1].copy())
        T2, W2 = run(sc, knn, "node_distance", 7.0, dtype, workspace=ws, rebuild_candidates=True)
        assert torch.equal(T2, T) and torch.equal(W2, Wt)
        Tk, Wk = k3(sc, knn, dtype, ws, False)
        assert torch.equal(Tk, Tf) and torch.equal(Wk, Wf)


# ---------------------------------------------------------------------------------------------- 5. slabs
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name,knn", [("main", 4), ("ragged", 3)])
def test_slabs_equal_the_whole_grid(name, knn, dtype):
    sc = scene_of(name)
    shape = sc["shape"]
    N = len(sc["node_pos"])
    T, Wt = run(sc, knn, "node_distance", 7.0, dtype)
    T0, W0 = WN.start_volumes(sc, dtype)
    T2, W2 = dev(T0), dev(W0)
    for (a, b), level in (((0, 5), 0), ((5, shape[0]), 1)):
        ws = kernels.dqb_workspace(shape, (a, b)) if level == 0 else kernels.dqb_workspace(shape, (a, b), knn=knn, n_nodes=N, level=1)
        for rebuild in (True, False):
            Ts, Ws = dev(T0[a:b]), dev(W0[a:b])
            run(sc, knn, "node_distance", 7.0, dtype, T=Ts, Wt=Ws, res=shape, x_range=(a, b), workspace=ws, rebuild_candidates=rebuild)
        T2[a:b] = Ts
        W2[a:b] = Ws
    assert torch.equal(T2, T) and torch.equal(W2, Wt)


def test_an_empty_slab_touches_nothing():
    sc = scene_of("main")
    Te = torch.empty((0, 32, 32), dtype=torch.float32, device="cuda")
    ws = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    out = run(sc, 4, T=Te, Wt=Te.clone(), res=(32, 32, 32), x_range=(9, 9), workspace=ws)
    assert out[0] is Te and bool((ws == -7).all())
    # no views: nothing is touched either
    T, Wt = run(sc, 4, depths=[], lws=[], workspace=ws)
    T0, _ = WN.start_volumes(sc)
    assert bool((T == dev(T0)).all()) and bool((Wt == 0).all()) and bool((ws == -7).all())


# ---------------------------------------------------------------------------------------------- the reference-shaped class
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fusion_update_tsdf_depths(dtype):
    """Fusion.updateTSDF_depths is the kernel call on the object's volumes, nodes and `_lw`; its second call loads the
    neighbourhoods its first one stored; maps that are not float32-exact travel as float64."""
    from dynamicfusion_body_amd import Fusion
    sc = scene_of("main")
    T0, W0 = WN.start_volumes(sc, dtype)
    f = Fusion(T0.copy(), sc["tdist"], knn=4, volume_dtype=dtype)
    f._tsdfw = W0
    f._K, f._Kinv = sc["K"], sc["Kinv"]
    f._nodes = [(0, sc["node_pos"][i], sc["node_dq"][i], float(sc["node_w"][i])) for i in range(len(sc["node_pos"]))]
    f._lw = sc["lw_dq"]
    f.updateTSDF_depths(sc["depths"], sc["lws"], wmax=7.0, scale=sc["scale"], center=sc["center"])
    T, Wt = run(sc, 4, "node_distance", 7.0, dtype)
    assert torch.equal(f._T, T) and torch.equal(f._Wt, Wt) and (Wt != 0).sum() > 15000
    fine = [d.astype(np.float64) * (1 + 2.0 ** -30) for d in sc["depths"]]               # not float32-exact
    f.updateTSDF_depths(fine, sc["lws"], wmax=7.0, weight="unit", scale=sc["scale"], center=sc["center"])
    run(sc, 4, "unit", 7.0, dtype, depths=fine, T=T, Wt=Wt)
    assert torch.equal(f._T, T) and torch.equal(f._Wt, Wt)
