"""GPU: the float32 instances of K2 (FusionDM.updateTSDF) and K3 (Fusion.updateTSDF) that bench.py and the frame loop run, against
the fp64 C oracle (oracle/oracle_c.c: oracle_np.update_tsdf_rigid / update_tsdf_dqb restated), every voxel at the sizes they run
(512^3 K3: every voxel of a seeded sample of whole bricks).

Every call is judged on its own: the oracle starts from the device state just before that call, widened to float64 (inputs are
float32-exact: volumes and live as stored).  Bars (as test_dqb_live_volume_of_another_size_vs_oracle):
voxels outside the oracle's update mask keep their bits; K2 weights identical (as stored: the float32 rounding of the oracle's
1 + w, which is exact for the integer weights of K2 alone); K3 weights and all T within f32_tol(1) * (1 + |x|).

The instances (csrc/dfh_fuse_volume.hip, host side of dfh_fuse_volume_rigid / dfh_fuse_volume_dqb):
  K2  fuse_volume_rigid_fast_kernel<LiveT, STRIDED = Z / 4 % 64 == 0, NT = option k2_nt or a slab pair of volumes > 256 MB>;
  K3  store pass: fuse_volume_dqb_fast_kernel mode 1; steady state (mode 3, Z % 64 == 0): fuse_volume_dqb_lds_kernel (80 B/node
      table to 819 nodes, 64 B/node to 2 304, beyond: the plain fast kernel) + dqb_redo_kernel, and with the constant-live skip
      (option k3_skip, default on beyond 2^24 voxels) dqb_live_mask / reach / bound / stream<NT> in front.
"""
import os

import numpy as np
import pytest
import torch

from oracle import oracle_c as C
from oracle import oracle_np as O
from dynamicfusion_body_amd import _lib, kernels, scene
from dynamicfusion_body_amd.dq import twist_exp_dq
from test_gpu_fuse_volume import _skip_scene, f32_tol, small_dq

pytestmark = pytest.mark.gpu

NT = max(1, min(16, len(os.sched_getaffinity(0))))                                   # oracle threads
IDENT = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
LW_BENCH = np.array([0.9999995, 0.0005, -0.0007, 0.0004, 0.0, 0.05, -0.03, 0.02])   # bench.py k23_of's lw_rigid
_QZ = np.array([np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)])


def quarter_turn(t):
    """A quarter turn about z, then an integer translation t: samples land within rounding of lattice points."""
    return np.concatenate([_QZ, 0.5 * O.quaternion_multiply(np.array([0.0, *t], dtype=np.float64), _QZ)])


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    C.build()
    C.load()


def host64(t):
    return t.double().cpu().numpy()


def assert_matches(Tg, Wg, T0, W0, To, Wo, mask, w_exact, what):
    """Tg/Wg: the kernel's result, T0/W0: the state before the call, To/Wo/mask: the oracle's (all float64 numpy, one layout)."""
    keep = ~mask
    assert np.array_equal(Tg[keep], T0[keep]) and np.array_equal(Wg[keep], W0[keep]), ("voxels outside the update mask changed", what,
                                                                                      int(((Tg != T0) | (Wg != W0))[keep].sum()))
    for name, g, o, exact in (("w", Wg, Wo, w_exact), ("T", Tg, To, False)):
        bad = (g != o.astype(np.float32)) if exact else (np.abs(g - o) > f32_tol(1) * (1 + np.abs(o)))
        if bad.any():
            i = np.unravel_index(int(np.flatnonzero(bad)[0]), bad.shape)
            raise AssertionError("%s: %s off at %d voxels, first %s: kernel %r oracle %r (before %r / %r, mask %s)"
                                 % (what, name, int(bad.sum()), i, g[i], o[i], T0[i], W0[i], bool(mask[i])))


def live_volume(shape, centre, radius, tdist, dtype, seed=0):
    """A sphere's truncated distance with a little noise, float32-exact, on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    gx, gy, gz = (torch.arange(s, device="cuda", dtype=torch.float64) for s in shape)
    d = torch.sqrt((gx[:, None, None] - centre[0]) ** 2 + (gy[None, :, None] - centre[1]) ** 2 + (gz[None, None, :] - centre[2]) ** 2)
    v = torch.clamp(d - radius, -1.5 * tdist, 1.5 * tdist) + 0.01 * torch.randn(shape, device="cuda", dtype=torch.float64, generator=g)
    return v.float().to(dtype).contiguous()


# ------------------------------------------------------------------------------------------------------------------------- K2
def k2_check(T0, W0, live, lw, tdist, wmax, res, x_range=None, chunk=64):
    """One K2 call on copies of the slab T0/W0 (float32, device), compared with the oracle over every voxel, `chunk` planes at a
    time (host memory: the live volume + a few chunks).  Returns the number of updated voxels."""
    a, b = (0, res[0]) if x_range is None else x_range
    T, W = T0.clone(), W0.clone()
    kernels.fuse_volume_rigid(T, W, live, lw, tdist, wmax, res=res, x_range=(a, b))
    torch.cuda.synchronize()
    live_np = live.cpu().numpy()
    n = 0
    for c in range(a, b, chunk):
        e = min(b, c + chunk)
        Ti, Wi = host64(T0[c - a:e - a]), host64(W0[c - a:e - a])
        To, Wo = Ti.copy(), Wi.copy()
        nc, mask = C.update_tsdf_rigid(To, Wo, live_np, lw, tdist, wmax, x_base=c, return_mask=True, n_threads=NT)
        assert_matches(host64(T[c - a:e - a]), host64(W[c - a:e - a]), Ti, Wi, To, Wo, mask, True, ("K2", res, (c, e)))
        n += nc
    return n


def k2_state(res, tdist, seed):
    c = np.array(res) / 2.0
    gx, gy, gz = (torch.arange(s, device="cuda", dtype=torch.float32) for s in res)
    d = torch.sqrt((gx[:, None, None] - c[0]) ** 2 + (gy[None, :, None] - c[1]) ** 2 + (gz[None, None, :] - c[2]) ** 2)
    T0 = torch.clamp(d - 0.31 * min(res), -tdist, tdist).contiguous()
    g = torch.Generator(device="cuda").manual_seed(seed)
    W0 = torch.randint(0, 6, res, device="cuda", generator=g).float()                 # (zeros, and wmax = 5 reached)
    return T0, W0


K2_LW = {"bench": LW_BENCH, "scaled": small_dq(np.random.default_rng(3), 0.02, 0.4, 0.97), "identity": IDENT,
         "quarter": None}


@pytest.mark.parametrize("lw_kind", list(K2_LW))
@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("live_dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("res", [(64, 64, 256), (40, 36, 512)])
def test_k2_strided_vs_oracle(res, live_dtype, nt, lw_kind):
    """The strided instances (Z / 4 % 64 == 0), cached and non-temporal, float32 and float64 live, on the bench's lw_rigid, a
    non-unit lw (scale 0.97), the exact identity (every voxel through the fast kernel's redo branch) and a quarter turn about z plus
    an integer translation (near-lattice ties)."""
    tdist = 4.0
    T0, W0 = k2_state(res, tdist, 1)
    live = live_volume(res, np.array(res) / 2.0 + np.array([0.4, -0.3, 0.6]), 0.3 * min(res), tdist, live_dtype)
    lw = K2_LW[lw_kind] if lw_kind != "quarter" else quarter_turn((res[1] - 1, 0.0, 0.0))
    _lib.set_option("k2_nt", nt)
    n = k2_check(T0, W0, live, lw, tdist, 5.0, res)
    assert n > 0.3 * T0.numel(), n


@pytest.mark.parametrize("live_res", [(56, 36, 300), (40, 44, 200)])
@pytest.mark.parametrize("nt", [0, 1])
def test_k2_slabs_and_live_of_another_size_vs_oracle(live_res, nt):
    """A live volume larger / smaller than the grid on every axis, and slabs (one starting at x0 = 13, not a multiple of 4)."""
    res, tdist = (48, 40, 256), 4.0
    T0, W0 = k2_state(res, tdist, 2)
    live = live_volume(live_res, np.array(res) / 2.0 + 0.4, 0.3 * min(res), tdist, torch.float32)
    lw = small_dq(np.random.default_rng(7), 0.02, 0.5)
    _lib.set_option("k2_nt", nt)
    n = 0
    for a, b in ((0, 13), (13, 30), (30, 48)):
        n += k2_check(T0[a:b].contiguous(), W0[a:b].contiguous(), live, lw, tdist, 5.0, res, x_range=(a, b))
    assert n > 0.3 * T0.numel(), n


@pytest.mark.parametrize("R", [256, 512])
def test_k2_whole_grid_vs_oracle(R):
    """256^3 and 512^3 whole grids on the library's own choice of instance (512^3: the non-temporal one), the bench's lw_rigid."""
    res, tdist = (R, R, R), 4.0
    T0, W0 = k2_state(res, tdist, 3)
    live = live_volume(res, np.array(res) / 2.0 + np.array([0.4, -0.3, 0.6]), 0.3 * R, tdist, torch.float32)
    n = k2_check(T0, W0, live, LW_BENCH, tdist, 5.0, res, chunk=32)
    assert n > 0.5 * T0.numel(), n


# ------------------------------------------------------------------------------------------------------------------------- K3
def k3_call(T, W, live, live_np, nodes, k, lw, tdist, wmax, res, x_range, ws, rebuild, what):
    """One K3 call on the device slab T/W (in place), compared over every voxel with the oracle started from the state before it.
    Returns the number of updated voxels."""
    a, b = x_range
    T0, W0 = host64(T), host64(W)
    kernels.fuse_volume_dqb(T, W, live, *nodes, k, lw, tdist, wmax, res=res, x_range=x_range, workspace=ws, rebuild_candidates=rebuild)
    torch.cuda.synchronize()
    To, Wo = T0.copy(), W0.copy()
    n, mask = C.update_tsdf_dqb(To, Wo, live_np, *(x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in nodes), k, lw, tdist,
                                wmax, x_base=a, return_mask=True, n_threads=NT)
    assert_matches(host64(T), host64(W), T0, W0, To, Wo, mask, False, what)
    return n


def k3_run(res, N, tdist, field, live_dtype=torch.float32, lw=IDENT, slabs=None, live_res=None, seed=3):
    """The store call, two steady-state calls, then one on the initial volumes again, per slab, each against the oracle.  Returns
    [(slab, workspace, updated counts)]."""
    k, wmax = 4, 9.0
    torch.manual_seed(seed)
    live, T0, W0, node_pos, node_w, dqs = _skip_scene(res, N, tdist, "gentle" if field == "random" else field, seed=seed,
                                                      live_res=live_res)
    if field == "random":                                                   # rotations and translations of a few tenths of a voxel
        rng = np.random.default_rng(seed)
        dqs = twist_exp_dq(rng.normal(size=(N, 6)) * np.array([.02, .02, .02, .4, .4, .4]))
    live = live.to(live_dtype)
    live_np = live.cpu().numpy()
    out = []
    for a, b in slabs or ((0, res[0]),):
        ws = kernels.dqb_workspace(res, (a, b), knn=k, n_nodes=N, level=2)
        T, W = T0[a:b].clone(), W0[a:b].clone()
        counts = [k3_call(T, W, live, live_np, (node_pos, dqs, node_w), k, lw, tdist, wmax, res, (a, b), ws, rebuild,
                          (res, N, field, (a, b), i)) for i, rebuild in enumerate((True, False, False))]
        # ... and a steady call on volumes the store pass never saw (w = 0 again where the live volume is constant: the first-touch
        # rule inside the stream and the LDS kernel, which the frame loop's own sequence never reaches there)
        T, W = T0[a:b].clone(), W0[a:b].clone()
        counts.append(k3_call(T, W, live, live_np, (node_pos, dqs, node_w), k, lw, tdist, wmax, res, (a, b), ws, False,
                              (res, N, field, (a, b), "fresh volumes")))
        out.append(((a, b), ws, counts))
        assert min(counts) > 1000, counts
    return out


K3_LDS_CASES = {  # name: (res, N, tdist, field, live dtype, lw, k3_tpb)
    "64-150-random-lw": ((64, 64, 64), 150, 3.0, "random", torch.float32, "random", None),
    "128-150-f64-live": ((128, 128, 128), 150, 4.0, "gentle", torch.float64, None, None),
    "256-512-config3": ((256, 256, 256), 512, 4.0, "gentle", torch.float32, None, None),
    "64-819-80B": ((64, 64, 64), 819, 3.0, "random", torch.float32, "random", None),
    "64-820-64B": ((64, 64, 64), 820, 3.0, "random", torch.float32, "random", None),
    "64-2304-64B": ((64, 64, 64), 2304, 3.0, "random", torch.float32, "random", None),
    "64-2305-plain": ((64, 64, 64), 2305, 3.0, "random", torch.float32, "random", None),
    "64-150-tpb256": ((64, 64, 64), 150, 4.0, "gentle", torch.float32, "random", 256),
    "64-150-tpb512": ((64, 64, 64), 150, 4.0, "gentle", torch.float64, None, 512),
    "64-150-identity": ((64, 64, 64), 150, 2.0, "identity", torch.float32, None, None),
    "ragged-y62": ((64, 62, 128), 150, 3.0, "gentle", torch.float32, "random", None),
}


@pytest.mark.parametrize("case", list(K3_LDS_CASES))
def test_k3_lds_kernel_vs_oracle(case):
    """The store pass and two steady-state calls through the LDS kernel and its redo list (skip off), against the oracle: 64^3 /
    150 nodes, 128^3, config 3's 256^3 / 512 Fibonacci nodes, node counts at the LDS table's limits (819 | 820: 80 -> 64 B per
    node; 2 304 | 2 305: beyond the table, the plain fast kernel), workgroups of 256 / 512 / 1024 threads, float32 and float64
    live, the identity field (every voxel on the redo list), a ragged y extent, non-identity lw; W0 holds zeros (first touch)
    and saturated weights (wmax = 9) throughout."""
    res, N, tdist, field, live_dtype, lw_kind, tpb = K3_LDS_CASES[case]
    lw = small_dq(np.random.default_rng(11), 0.01, 0.3, 0.99) if lw_kind == "random" else IDENT
    _lib.set_option("k3_skip", 0)
    if tpb is not None:
        _lib.set_option("k3_tpb", tpb)
    k3_run(res, N, tdist, field, live_dtype, lw)


def test_k3_slabs_vs_oracle():
    """Slabs of one grid with the skip forced on: [0, 24) may skip; [24, 37) (a plane count not a multiple of 4) and [37, 64)
    (x0 % 4 != 0) rule it out and run the LDS kernel alone."""
    _lib.set_option("k3_skip", 1)
    res, N = (64, 64, 128), 150
    shares = []
    for (a, b), ws, _ in k3_run(res, N, 4.0, "gentle", slabs=((0, 24), (24, 37), (37, 64))):
        tabs = kernels.dqb_skip_tables(ws, res, res, N, x_range=(a, b))
        shares.append(float(tabs["S"].float().mean()) if tabs["ok"] else None)
    assert shares[0] is not None and shares[0] > 0.05, shares


@pytest.mark.parametrize("R,tdist", [(64, 4.0), (64, 3.0), (128, 4.0), (128, 3.0), (256, 4.0), (256, 3.0)])
def test_k3_constant_live_skip_vs_oracle(R, tdist):
    """The constant-live skip forced on (k3_skip = 1): bricks that stream (dqb_stream_kernel) and bricks left to the LDS kernel,
    every voxel against the oracle; tdist 4 (a power of two with float-exact wmax: the stream's saturated shortcut) and 3 (none)."""
    _lib.set_option("k3_skip", 1)
    res, N = (R, R, R), 150 if R < 256 else 512
    (_, ws, _), = k3_run(res, N, tdist, "gentle")
    tabs = kernels.dqb_skip_tables(ws, res, res, N)
    assert tabs["ok"]
    S = tabs["S"].cpu().numpy()
    assert 16 <= int((S == 1).sum()) < S.size, S.mean()                    # streamed bricks are among those compared


@pytest.mark.parametrize("res,live_res", [((32, 32, 512), (32, 32, 192)), ((32, 32, 512), (32, 32, 256)), ((32, 32, 512), (32, 32, 320)),
                                          ((32, 32, 256), (32, 32, 384)), ((32, 32, 256), (24, 40, 256)), ((32, 32, 256), (40, 22, 200))])
def test_k3_constant_live_skip_with_a_live_volume_of_another_size_vs_oracle(res, live_res):
    """The live extents of test_dqb_constant_live_skip_with_a_live_volume_of_another_size, against the oracle instead of skip off."""
    _lib.set_option("k3_skip", 1)
    N = 150
    (_, ws, _), = k3_run(res, N, 4.0, "gentle", live_res=live_res)
    tabs = kernels.dqb_skip_tables(ws, res, live_res, N)
    assert tabs["ok"] and float(tabs["S"].float().mean()) > 0.05


def test_k3_512_2048_nodes_sampled_bricks_vs_oracle():
    """The bench's second k23 size: 512^3, 2 048 Fibonacci nodes (64 B/node LDS table), skip on by default, dqb_stream_kernel<true>.
    A store call, a steady call and a steady call on the initial volumes (w = 0 in streamed bricks), each compared on every voxel of a seeded sample of 1/64 of the 4 x 4 x 16 bricks (oracle form
    (b)); the sample holds bricks that streamed and bricks that went through the warp kernel."""
    res, N, k, tdist, wmax = (512, 512, 512), 2048, 4, 4.0, 9.0
    torch.manual_seed(5)
    live, T, W, node_pos, node_w, dqs = _skip_scene(res, N, tdist, "gentle")
    live_np = live.cpu().numpy()
    nb = (res[0] // 4, res[1] // 4, res[2] // 16)
    bricks = np.sort(np.random.default_rng(64).choice(nb[0] * nb[1] * nb[2], size=nb[0] * nb[1] * nb[2] // 64, replace=False))
    bx, by, bz = np.unravel_index(bricks, nb)
    ox, oy, oz = np.meshgrid(np.arange(4), np.arange(4), np.arange(16), indexing="ij")
    idx = (((bx[:, None] * 4 + ox.reshape(-1)) * res[1] + (by[:, None] * 4 + oy.reshape(-1))) * res[2]
           + (bz[:, None] * 16 + oz.reshape(-1))).reshape(-1)
    idx_d = torch.from_numpy(idx).cuda()
    ws = kernels.dqb_workspace(res, knn=k, n_nodes=N, level=2)
    T0, W0 = T.clone(), W.clone()
    for rebuild in (True, False, None):                                    # store, steady, steady on the initial volumes again
        if rebuild is None:
            T, W, rebuild = T0, W0, False
        Ti, Wi = T.view(-1)[idx_d].double().cpu().numpy(), W.view(-1)[idx_d].double().cpu().numpy()
        kernels.fuse_volume_dqb(T, W, live, node_pos, dqs, node_w, k, IDENT, tdist, wmax, workspace=ws, rebuild_candidates=rebuild)
        torch.cuda.synchronize()
        To, Wo, mask = C.update_tsdf_dqb_at(idx, res, Ti, Wi, live_np, node_pos, dqs, node_w, k, IDENT, tdist, wmax, n_threads=NT)
        assert_matches(T.view(-1)[idx_d].double().cpu().numpy(), W.view(-1)[idx_d].double().cpu().numpy(), Ti, Wi, To, Wo, mask,
                       False, ("K3 512^3", rebuild, T is T0))
        assert int(mask.sum()) > 100000
    S = kernels.dqb_skip_tables(ws, res, res, N)["S"].cpu().numpy()
    assert S.size == bricks.size * 64
    assert (S[bricks] == 1).sum() > 100 and (S[bricks] == 0).sum() > 100, (S[bricks] == 1).mean()


# ------------------------------------------------------------------------------------------------------------- the bench's state
def test_k23_on_the_frame_loops_state_vs_oracle():
    """bench.py k23_of on a 256^3 SlabFrame after three frames: one K2 call with lw_rigid and one steady K3 call (skip off and
    skip on) on clones of the canonical volume, with the loop's live volume, node DQs and stored neighbourhoods -- exactly the
    work k23 times, every voxel against the oracle."""
    from dynamicfusion_body_amd.pipeline import SlabFrame
    R, N = 256, 512
    H, Wd, fx, cx, cy = scene.CAMERAS["C2"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=4.0, distributed=False)
    lws = [scene.view_extrinsic(a) for a in (0.0, 40.0, -40.0)]
    for lw in lws:
        sf.integrate(torch.from_numpy(scene.render_depth(K, lw, H, Wd, dtype=np.float32, invalid_frac=0.0)).cuda(), lw)
    sf.refresh_samples()
    for f in range(3):
        off = np.array([0.10, -0.07, 0.05]) * (f + 1) * scale
        ds = [torch.from_numpy(scene.render_depth(K, lw, H, Wd, dtype=np.float32, invalid_frac=0.0, sphere_offset=off,
                                                  sphere_r=scene.SPHERE_R * (1.0 + 0.004 * (f + 1)))).cuda() for lw in lws]
        sf.step(ds, lws, gn_iters=10)
    torch.cuda.synchronize()
    res, tv = (R, R, R), sf.tvox
    sv = sf.fs.solver
    assert float((sv.node_dq[:, 4:].abs()).max()) > 1e-4                   # the warp field is not the identity
    n = k2_check(sf.T.clone(), sf.Wt.clone(), sf.live, LW_BENCH, tv, 100.0, res, x_range=(sf.a, sf.b), chunk=64)
    assert n > 0.1 * sf.T.numel(), n
    live_np = sf.live.cpu().numpy()
    for skip in (0, 1):
        _lib.set_option("k3_skip", skip)
        T, W = sf.T.clone(), sf.Wt.clone()
        n = k3_call(T, W, sf.live, live_np, (sv.node_pos, sv.node_dq, sv.node_w), sf.knn, sf.ident_lw, tv, 100.0, res, (sf.a, sf.b),
                    sf.ws_dqb, False, ("k23 state", skip))
        assert n > 0.1 * T.numel(), n
        if skip:
            tabs = kernels.dqb_skip_tables(sf.ws_dqb, res, res, N, x_range=(sf.a, sf.b))
            assert tabs["ok"] and float(tabs["S"].float().mean()) > 0.05
