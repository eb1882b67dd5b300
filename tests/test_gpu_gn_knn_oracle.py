"""GPU: the node iterations' normal-equation build at every knn (1 .. 8) against the fp64 oracle (oracle/gn_np.py).

The data-row kernel (gn_build_data_kernel<K, PLANNED, ASSOC>), the gather (gn_gather_kernel<K>) and the regulariser's pair rows
are compiled once per K; the MFMA Gram tiling (ceil((6K + 1) / 16) tiles per side), the scratch-row layout and the list
entries all depend on K.  Elsewhere the assembled system meets the oracle at K = 4 only.  Here:

  1. every build path (planned, atomic, regulariser in its own gather / own launch) at K = 1 .. 8, on ragged sample counts,
     an all-invalid tile, nodes without samples, exact distance ties and lists beyond 256 entries;
  2. the fused-association builds (one view, three views) at K = 1 .. 8: bit for bit the separate path, the upper-triangle
     gather bit for bit the full one, and both against the oracle's association and system;
  3. K = 8 at N = 215 (tuple keys packed on the device, just under 2^62) and N = 216 (torch.unique, no keys), and a second
     sample set on the kept pattern;
  4. the one-call GN loop (dfh_gn_solve) at knn 3 and 8 against gn_loop_truncated;
  5. dfh_gn_solve with n_global > 0 (n_global rigid-mode steps + the node iterations) against the separate calls and the oracle.

Bounds of the system, per entry: |A - A_o| <= 1e-10 A_abs + 1e-13 max(A_abs), where A_abs is the same assembly of |J| and |r|
(a single max-relative bound would hide a missing low-weight contribution); entries with A_abs = 0 are exactly 0; J^T r to
1e-10 of its largest entry; the objective to 1e-12 relative; the valid count exact.  Each test prints what it achieved (-s).
"""
import numpy as np
import pytest
import torch

from oracle import gn_np as G
from oracle import oracle_np as O
from dynamicfusion_body_amd import _lib, kernels, scene, solve
from dynamicfusion_body_amd.pipeline import FrameSolver

pytestmark = pytest.mark.gpu

IDENT = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
KNNS = list(range(1, 9))
LW = 1.03 * G.twist_exp_dq(np.array([0.01, -0.02, 0.015, 0.3, -0.2, 0.1]))          # a global warp with |r_lw| = 1.03


# ---------------------------------------------------------------- oracle side and the comparison
def oracle_system(dq, pos, nrm, corr, valid, nbr, node_nbr, node_pos, node_w, lw, rw, huber):
    """The oracle's normal equations of a build: (keys, blocks, blocks of |J| and |r|, J^T r (N,6), objective, valid count) --
    the data rows of the valid samples, Huber-weighted as the builds weight them, and the regulariser's pair rows."""
    N = len(dq)
    sel = np.flatnonzero(valid)
    r, J = G.data_residual_jacobian(dq, pos[sel], nrm[sel], corr[sel], nbr[sel], node_pos, node_w, lw)
    obj = 0.5 * float(r @ r)
    if huber > 0.0:
        sc, obj = G.huber_scale(r, huber)
        r, J = r * sc, J * sc[:, None, None]
    rho, nb, Ji, Jj = G.reg_residual_jacobian(dq, np.arange(N), node_nbr, node_pos, node_w, rw)
    keys, A, b, _ = G.assemble_blocks(N, r, J, nbr[sel], rho, nb, Ji, Jj)
    keys_a, A_abs, _, _ = G.assemble_blocks(N, np.abs(r), np.abs(J), nbr[sel], np.abs(rho), nb, np.abs(Ji), np.abs(Jj))
    assert np.array_equal(keys, keys_a)
    return keys, A, A_abs, b, obj + 0.5 * float(np.sum(rho * rho)), len(sel)


def check_system(sv, ref, tag):
    """The solver's last build against oracle_system's: returns the largest entrywise ratio |A - A_o| / bound."""
    keys_o, A_o, A_abs, b_o, cost_o, cnt_o = ref
    N = sv.N
    keys = np.repeat(np.arange(N, dtype=np.int64), np.diff(sv.row_ptr.cpu().numpy())) * N + sv.col.cpu().numpy().astype(np.int64)
    A = sv.vals.cpu().numpy().reshape(-1, 6, 6)
    b = sv.rhs.cpu().numpy().reshape(N, 6)
    cost, cnt = sv.cost()
    assert cnt == cnt_o, (tag, cnt, cnt_o)
    assert abs(cost - cost_o) <= 1e-12 * cost_o, (tag, cost, cost_o)
    assert np.abs(b - b_o).max() <= 1e-10 * np.abs(b_o).max(), tag
    # structure: every block the oracle assembles is in the pattern ...
    at = np.minimum(np.searchsorted(keys, keys_o), len(keys) - 1)
    assert np.array_equal(keys[at], keys_o), (tag, "a block is missing from the pattern")
    Ao, Aa = np.zeros_like(A), np.zeros_like(A)
    Ao[at], Aa[at] = A_o, A_abs
    # ... and an entry no row reaches (A_abs = 0: head-room blocks, exact zeros of the Jacobians) is exactly 0
    assert (A[Aa == 0.0] == 0.0).all(), (tag, "non-zero entry where no row contributes")
    ratio = np.abs(A - Ao) / (1e-10 * Aa + 1e-13 * Aa.max())
    worst = float(ratio.max())
    assert worst <= 1.0, (tag, worst, np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    return worst


def host(sv):
    """The solver's sorted samples and its graph as numpy: (pos, nrm, nbr, node_nbr, corr, valid)."""
    return (sv.spos.cpu().numpy(), sv.snrm.cpu().numpy(), sv.snbr.cpu().numpy().astype(np.int64),
            sv.node_nbr.cpu().numpy().astype(np.int64), sv.corr.cpu().numpy(), sv.valid.cpu().numpy().astype(bool))


# ---------------------------------------------------------------- 1. every K, every build path
def field(N, rng):
    tw = rng.standard_normal((N, 6)) * np.array([0.02, 0.02, 0.02, 0.3, 0.3, 0.3])
    return G.apply_twists(np.tile(IDENT, (N, 1)), tw)


def unit_normals(S, rng):
    n = rng.standard_normal((S, 3))
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def problem(K, shape, rng):
    """(node_pos, node_w, node DQs, samples) of one synthetic problem."""
    if shape == "cluster":
        # N = K: every tuple holds every node.  A tight cluster is one tuple that fills whole tiles, the spread rest gives many
        # short runs; more than 256 rows reach every block, so the gather walks its lists in chunks
        N = K
        npos = rng.uniform(0, 12, size=(N, 3))
        nw = rng.uniform(4, 8, size=N)
        S = 128 * 262
        n_cl = int(0.9 * S)
        pts = np.concatenate([np.array([3.0, 4.0, 5.0]) + 0.05 * rng.standard_normal((n_cl, 3)), rng.uniform(-2, 14, size=(S - n_cl, 3))])
    else:
        # 50 nodes among the samples, 5 twins of them (exact distance ties: the lower index comes first), 6 far away (no data
        # sample reaches them; the regulariser joins them to the rest)
        npos = np.concatenate([rng.uniform(0, 40, size=(50, 3)), np.zeros((5, 3)), 200.0 + rng.uniform(0, 10, size=(6, 3))])
        twins = [3, 9, 17, 30, 44]
        npos[50:55] = npos[twins]
        nw = rng.uniform(8, 14, size=len(npos))
        nw[50:55] = nw[twins]
        pts = rng.uniform(0, 40, size=({"S1": 1, "S127": 127, "S129": 129, "S3000": 3000}[shape], 3))
    return npos, nw, field(len(npos), rng), pts


def make_solver(K, npos, nw, dq, pts, nrm):
    node_nbr, _ = solve.sample_knn(npos, npos, nw, K)
    sv = solve.WarpSolver(knn=K, pcg_iters=5, distributed=False)
    sv.set_graph(npos, dq, nw, node_nbr=node_nbr)
    sv.set_samples(pts, nrm)
    return sv


@pytest.mark.parametrize("shape", ["S1", "S127", "S129", "S3000", "cluster"])
@pytest.mark.parametrize("K", KNNS)
def test_build_every_knn_and_path_vs_oracle(K, shape):
    """Planned build, atomic build (dfh_gn_build without a plan), regulariser in its own gather and in its own launch, Huber 0 and a delta that
    down-weights 40 % of the rows: all against the oracle; the planned build twice: the same bits."""
    rng = np.random.default_rng(100 * K + ["S1", "S127", "S129", "S3000", "cluster"].index(shape))
    npos, nw, dq, pts = problem(K, shape, rng)
    S = len(pts)
    nrm = unit_normals(S, rng)
    corr = pts + 0.3 * rng.standard_normal((S, 3))
    rw = 0.7
    sv = make_solver(K, npos, nw, dq, pts, nrm)
    order = sv._order_index().cpu().numpy()
    valid = rng.random(S) >= 0.4
    if S == 1:
        valid[:] = True
    if S >= 256:
        valid[order[128:256]] = False                            # the second tile (in sorted order): no valid sample at all
    sv.set_correspondences(corr, valid)
    pos, nrm_s, nbr, node_nbr, corr_s, valid_s = host(sv)
    # the samples' and the nodes' neighbours: k nearest, nearest first, exact ties to the lower index
    assert np.array_equal(nbr, O.knn_bruteforce(pos, npos, K))
    assert np.array_equal(node_nbr, O.knn_bruteforce(npos, npos, K))
    if shape == "S3000":
        assert K == 1 or ((nbr == 3).any(axis=1) & (nbr == 50).any(axis=1)).any()     # tuples that hold both twins of a tie
        assert not np.isin(np.arange(55, 61), nbr).any()                               # nodes without a data sample
        assert not valid_s[128:256].any() and valid_s.any()
    ref0 = oracle_system(dq, pos, nrm_s, corr_s, valid_s, nbr, node_nbr, npos, nw, LW, rw, 0.0)
    r_valid, _ = G.data_residual_jacobian(dq, pos[valid_s], nrm_s[valid_s], corr_s[valid_s], nbr[valid_s], npos, nw, LW)
    delta = float(np.percentile(np.abs(r_valid), 60))
    if len(r_valid) >= 50:
        assert 0.2 <= (np.abs(r_valid) > delta).mean() <= 0.6
    ref1 = oracle_system(dq, pos, nrm_s, corr_s, valid_s, nbr, node_nbr, npos, nw, LW, rw, delta)
    worst = {}
    for huber, ref in ((0.0, ref0), (delta, ref1)):
        tag = (K, shape, huber)
        sv.build(LW, rw, huber)
        worst["planned"] = max(worst.get("planned", 0.0), check_system(sv, ref, tag + ("planned",)))
        s1 = sv.system.clone()
        sv.build(LW, rw, huber)
        assert torch.equal(s1, sv.system), tag                  # no atomics in the planned build: the same bits
        # the regulariser's lists walked in a gather of their own: the same sums in the same order -- the same bits -- while every
        # regulariser list is at most kCoopList (12, csrc/dfh_solve.hip) long and every data list at most 256.  Beyond, the two
        # gathers add the regulariser's list in different orders (own gather: a long list split among four waves; fused: beside
        # a data list of > 256 entries, the sequential walk): the same sums to rounding, checked against the oracle
        same_order = int(np.diff(sv.rblk_ptr.cpu().numpy()).max()) <= 12 and int(np.diff(sv.blk_ptr.cpu().numpy()).max()) <= 256
        for switch in ("gn_reg_own_gather", "gn_reg_own_launch"):
            _lib.set_option(switch, 1)
            sv.build(LW, rw, huber)
            _lib.set_option(switch, None)
            worst[switch] = max(worst.get(switch, 0.0), check_system(sv, ref, tag + (switch,)))
            assert torch.equal(s1, sv.system) or not same_order, tag + (switch,)
        if huber == 0.0:
            _lib.set_option("py_gn_atomic", 1)                  # the atomic dfh_gn_build (for K > 4 its table-less branch)
            sv.build(LW, rw, huber)
            worst["atomic"] = check_system(sv, ref, tag + ("atomic",))
            with pytest.raises(ValueError):
                sv.build(LW, rw, delta)                         # the atomic build has no Huber weights: refused, not ignored
            _lib.set_option("py_gn_atomic", None)
    if shape == "cluster":
        assert np.diff(sv.blk_ptr.cpu().numpy()).max() > 256                          # the chunked walk
        assert (np.diff(sv._row_first.cpu().numpy()) == 128).any()                     # one tuple fills a whole tile
    print("K=%d %s: largest |A - A_o| / bound %s" % (K, shape, {k: "%.3g" % v for k, v in worst.items()}))


# ---------------------------------------------------------------- the R = 64 sphere scene (sections 2, 4, 5)
_SCENE = {}
RW, LM_ABS, LM_REL, GATE, HUBER, PCG = 5.0, 10.0, 1e-2, 2.0, 0.5, 10          # the benched settings (bench.py gn leg)


def sphere_scene():
    """test_multi_view_association_and_gn_loop_vs_oracle's scene: a sphere fused from five views at R = 64, 96 Fibonacci nodes,
    three live views 50 degrees apart of the sphere displaced by (0.5, -0.35, 0.25) voxels and inflated by 2 %, a moved field."""
    if not _SCENE:
        R, N = 64, 96
        H, W, fx, cx, cy = scene.CAMERAS["C1"]
        K = scene.intrinsics(fx, cx, cy)
        Kinv = np.linalg.inv(K)
        scale, center, tdist = scene.grid_params(R)
        T = torch.full((R, R, R), tdist, dtype=torch.float32, device="cuda")
        Wt = torch.zeros_like(T)
        for a in (0.0, 50.0, -50.0, 130.0, -130.0):
            lw = scene.view_extrinsic(a)
            d = torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda()
            kernels.integrate_depth(T, Wt, d, K, Kinv, lw, scale, center, tdist)
        node_pos, node_w = scene.fibonacci_nodes(N, R)
        off = np.array([0.5, -0.35, 0.25]) * scale
        lws = [scene.view_extrinsic(a) for a in (0.0, 50.0, -50.0)]
        lives = [scene.render_depth(K, lw, H, W, dtype=np.float32, sphere_offset=off, sphere_r=scene.SPHERE_R * 1.02) for lw in lws]
        dq1 = G.apply_twists(np.tile(IDENT, (N, 1)), np.random.default_rng(11).normal(scale=[2e-3] * 3 + [0.15] * 3, size=(N, 6)))
        _SCENE.update(R=R, N=N, K=K, Kinv=Kinv, scale=scale, center=center, T=T, Wt=Wt, node_pos=node_pos, node_w=node_w, lws=lws,
                      lives=lives, depths=[torch.from_numpy(d).cuda() for d in lives], dq1=dq1)
    return _SCENE


def scene_solver(knn):
    s = sphere_scene()
    fs = FrameSolver(s["K"], s["scale"], s["center"], s["R"] / 2, knn=knn, pcg_iters=PCG, distributed=False)
    fs.set_graph(s["node_pos"], np.tile(IDENT, (s["N"], 1)), s["node_w"])
    assert fs.set_canonical(s["T"], s["Wt"], band=2.0) > 2000
    return fs


# ---------------------------------------------------------------- 2. the fused-association builds at every K
@pytest.mark.parametrize("K", KNNS)
def test_fused_association_builds_every_knn(K):
    """dfh_gn_build with a frame (one view, three views) after moving the field: corr, valid
    and the system bit for bit those of the separate association + planned build, the upper-triangle gather bit for bit the
    full one, corr / valid those of associate_depth_views on the oracle's warped samples, the system the oracle's."""
    s = sphere_scene()
    fs = scene_solver(K)
    sv = fs.solver
    dq1 = s["dq1"]
    worst = []
    for views in ((0,), (0, 1, 2)):
        arg_d = [s["depths"][v] for v in views] if len(views) > 1 else s["depths"][views[0]]
        arg_lw = [s["lws"][v] for v in views] if len(views) > 1 else s["lws"][views[0]]
        modes = ("fused", "separate") + (("full_gather",) if len(views) > 1 else ())
        snaps = {}
        for mode in modes:
            _lib.set_option("py_gn_no_fused_assoc", 1 if mode == "separate" else None)
            _lib.set_option("gn_gather_full", 1 if mode == "full_gather" else None)
            sv.node_dq.copy_(torch.from_numpy(dq1).cuda())
            sv.corr.zero_()
            sv.valid.zero_()
            sv.build_associated(arg_d, s["K"], s["Kinv"], arg_lw, s["scale"], s["center"], s["R"] / 2, fs.lw, RW, GATE, HUBER)
            snaps[mode] = (sv.corr.clone(), sv.valid.clone(), sv.vals.clone(), sv.rhs.clone(), sv.cost_count.clone())
        _lib.set_option("py_gn_no_fused_assoc", None)
        _lib.set_option("gn_gather_full", None)
        for mode in modes[1:]:
            for name, a, b in zip(("corr", "valid", "vals", "rhs", "cost_count"), snaps["fused"], snaps[mode]):
                assert torch.equal(a, b), (K, views, mode, name)
        pos, nrm, nbr, node_nbr, corr, valid = host(sv)
        warped = O.warp(pos, dq1[nbr], s["node_pos"][nbr], s["node_w"][nbr], m_lw=fs.lw)
        co, vo, view = G.associate_depth_views(warped, s["K"], s["Kinv"], [s["lws"][v] for v in views], [s["lives"][v] for v in views],
                                               s["scale"], s["center"], s["R"] / 2, GATE)
        assert np.array_equal(valid, vo), (K, views, int((valid != vo).sum()))
        assert vo.sum() > 1000 and (~vo).any()
        assert len(views) == 1 or len(set(view[vo])) == 3
        assert np.abs(corr - co).max() <= 1e-9, K
        ref = oracle_system(dq1, pos, nrm, co, vo, nbr, node_nbr, s["node_pos"], s["node_w"], fs.lw, RW, HUBER)
        worst.append(check_system(sv, ref, (K, views)))
    print("K=%d fused association: largest |A - A_o| / bound, one view %.3g, three views %.3g" % (K, worst[0], worst[1]))


# ---------------------------------------------------------------- 3. the tuple-key paths at knn 8
@pytest.mark.parametrize("N", [215, 216])
def test_knn8_tuple_keys_at_the_2_62_edge(N):
    """215^8 < 2^62 <= 216^8: at N = 215 the device packs the tuples into int64 keys (the device plan and the torch plan: the
    same lists, the same bits), at N = 216 set_samples groups them with torch.unique and the plan has no keys.  Both against the
    oracle by block key; at N = 216 a second sample set on the kept pattern, one it covers and one that makes it grow, equals a
    fresh solver's build bit for bit."""
    K = 8
    rng = np.random.default_rng(N)
    npos = rng.uniform(0, 60, size=(N, 3))
    nw = rng.uniform(6, 10, size=N)
    dq = field(N, rng)
    S = 3000
    pts = rng.uniform(0, 60, size=(S, 3)) * np.array([0.5, 1.0, 1.0])           # the half x < 30: the rest is new ground later
    nrm = unit_normals(S, rng)
    corr = pts + 0.3 * rng.standard_normal((S, 3))
    valid = rng.random(S) >= 0.4
    rw, huber = 0.7, 0.5
    packed = float(N) ** K < 2.0 ** 62
    assert packed == (N == 215)
    sv = make_solver(K, npos, nw, dq, pts, nrm)
    sv.set_correspondences(corr, valid)
    if packed:
        assert sv._tuple_key is not None and int(sv._tuple_key.max()) < 2 ** 62
    else:
        assert sv._tuple_key is None
    sv.build(LW, rw, huber)
    pos, nrm_s, nbr, node_nbr, corr_s, valid_s = host(sv)
    worst = [check_system(sv, oracle_system(dq, pos, nrm_s, corr_s, valid_s, nbr, node_nbr, npos, nw, LW, rw, huber), (K, N))]
    if packed:
        _lib.set_option("py_plan_torch", 1)
        tv = make_solver(K, npos, nw, dq, pts, nrm)
        tv.set_correspondences(corr, valid)
        tv.build(LW, rw, huber)
        _lib.set_option("py_plan_torch", None)
        assert torch.equal(sv._tuple_key, tv._tuple_key) and torch.equal(sv._order_index(), tv._order_index())
        assert torch.equal(sv.snbr, tv.snbr) and sv.n_rows == tv.n_rows and torch.equal(sv.run_id, tv.run_id)
        for name in ("blk_ptr", "blk_ent", "node_ptr", "node_ent", "rblk_ptr", "rblk_ent", "rnode_ptr", "rnode_ent"):
            assert torch.equal(getattr(sv, name), getattr(tv, name)), name
        assert torch.equal(sv.system, tv.system)
    else:
        keys0 = sv._pattern_keys.clone()
        half = rng.random(S) < 0.5
        for pts2, grows in ((pts[half], False), (np.concatenate([pts[half], rng.uniform(30, 60, size=(500, 3))]), True)):
            S2 = len(pts2)
            nrm2 = unit_normals(S2, rng)
            corr2 = pts2 + 0.3 * rng.standard_normal((S2, 3))
            valid2 = rng.random(S2) >= 0.4
            sv.set_samples(pts2, nrm2)
            sv.set_correspondences(corr2, valid2)
            sv.build(LW, rw, huber)
            assert sv._tuple_key is None
            assert torch.equal(sv._pattern_keys, keys0) != grows, grows
            fresh = make_solver(K, npos, nw, dq, pts2, nrm2)
            fresh.set_correspondences(corr2, valid2)
            fresh.build(LW, rw, huber)
            A, b = sv.dense_normal_equations()
            Af, bf = fresh.dense_normal_equations()
            assert np.array_equal(A, Af) and np.array_equal(b, bf), grows
            assert sv.cost() == fresh.cost()
            pos, nrm_s, nbr, node_nbr, corr_s, valid_s = host(sv)
            worst.append(check_system(sv, oracle_system(dq, pos, nrm_s, corr_s, valid_s, nbr, node_nbr, npos, nw, LW, rw, huber),
                                      (K, N, grows)))
    print("K=8 N=%d: largest |A - A_o| / bound %s" % (N, ["%.3g" % w for w in worst]))


# ---------------------------------------------------------------- 4. the one-call loop at knn 3 and 8
def loop_oracle(fs, iters, **kw):
    s = sphere_scene()
    pos, nrm, nbr, node_nbr, _, _ = host(fs.solver)

    def assoc(w):
        c, v, _ = G.associate_depth_views(w, s["K"], s["Kinv"], s["lws"], s["lives"], s["scale"], s["center"], s["R"] / 2, GATE)
        return c, v
    return G.gn_loop_truncated(np.tile(IDENT, (s["N"], 1)), pos, nrm, nbr, node_nbr, s["node_pos"], s["node_w"], IDENT, assoc, iters, RW,
                               LM_ABS, LM_REL, HUBER, PCG, **kw)


def check_loop(tag, costs, counts, dq, or_costs, or_counts, dq_or):
    """The bars of test_multi_view_association_and_gn_loop_vs_oracle: cost at every iteration to 1e-4 relative, node DQs to 1e-5,
    valid counts within 3."""
    rel = float((np.abs(np.array(costs) - np.array(or_costs)) / np.array(or_costs)).max())
    dqe = float(np.abs(dq - dq_or).max())
    dn = max(abs(a - b) for a, b in zip(counts, or_counts))
    print("%s: cost rel %.3g, node DQ %.3g, valid count %d apart" % (tag, rel, dqe, dn))
    assert rel <= 1e-4, (tag, costs, or_costs)
    assert dqe <= 1e-5, (tag, dqe)
    assert dn <= 3, (tag, counts, or_counts)


def gpu_loop(fs, iters, **kw):
    """FrameSolver.gn_iteration(n_iters = m) from the identity for m = 1 .. iters: ONE library call of m iterations each time;
    the m-th call's last build is the m-th iteration's (the calls are deterministic), so every iteration's cost is seen.
    Returns (costs, valid counts, node DQs after the last call)."""
    s = sphere_scene()
    sv = fs.solver
    costs, counts = [], []
    for m in range(1, iters + 1):
        sv.node_dq.copy_(torch.from_numpy(np.tile(IDENT, (s["N"], 1))).cuda())
        fs.gn_iteration(s["depths"], s["lws"], rw=RW, lm_abs=LM_ABS, lm_rel=LM_REL, max_dist=GATE, huber=HUBER, n_iters=m, **kw)
        c, n = sv.cost()
        costs.append(c)
        counts.append(n)
    return costs, counts, sv.node_dq.cpu().numpy()


@pytest.mark.parametrize("knn", [3, 8])
def test_one_call_gn_loop_vs_oracle(knn):
    """dfh_gn_solve with n_iters > 1 on three views, the benched settings, against gn_loop_truncated."""
    fs = scene_solver(knn)
    iters = 4
    costs, counts, dq = gpu_loop(fs, iters)
    check_loop(("dfh_gn_solve", knn), costs, counts, dq, *loop_oracle(fs, iters))
    assert costs[-1] / counts[-1] < costs[0] / counts[0]


# ---------------------------------------------------------------- 5. dfh_gn_solve with rigid-mode steps
@pytest.mark.parametrize("knn", [3, 4])
def test_frame_solve_views_vs_separate_calls_and_oracle(knn):
    """gn_iteration(..., n_global=2): two rigid-mode steps from the built normal equations, then the node iterations, in one
    library call (dfh_gn_solve, n_global > 0) -- bit for bit build_associated + global_step twice and then gn_iteration(n_iters),
    and the oracle's loop with global_iters = 2, global_sampled = False at the bars of the loop test."""
    s = sphere_scene()
    fs = scene_solver(knn)
    sv = fs.solver
    iters = 3
    costs, counts, dq = gpu_loop(fs, iters, n_global=2, global_lm=0.1)
    one = tuple(t.clone() for t in (sv.node_dq, sv.system, sv.corr, sv.valid, sv.global_xi))
    sv.node_dq.copy_(torch.from_numpy(np.tile(IDENT, (s["N"], 1))).cuda())
    for _ in range(2):
        sv.build_associated(s["depths"], s["K"], s["Kinv"], s["lws"], s["scale"], s["center"], s["R"] / 2, fs.lw, RW, GATE, HUBER)
        sv.global_step(0.1)
    fs.gn_iteration(s["depths"], s["lws"], rw=RW, lm_abs=LM_ABS, lm_rel=LM_REL, max_dist=GATE, huber=HUBER, n_iters=iters)
    for name, a, b in zip(("node_dq", "system", "corr", "valid", "global_xi"), one,
                          (sv.node_dq, sv.system, sv.corr, sv.valid, sv.global_xi)):
        assert torch.equal(a, b), (knn, name)
    assert float(one[4][:6].abs().max()) > 0.0                                   # (the rigid-mode steps did move the field)
    check_loop(("dfh_gn_solve n_global", knn), costs, counts, dq,
               *loop_oracle(fs, iters, global_iters=2, global_sampled=False, global_lm=0.1))
