"""GPU: the landmark term (csrc/dfh_landmarks.hip: gn_landmark_rows_kernel<K> + the data term's gather with accumulate) against its
restatement (tests/landmark_np.py), from the kernel up to SlabFrame.step.

The system after build + term is compared, dense, with the restatement's under tests/test_gpu_gn_knn_oracle.py's bars: per entry
|A - A_o| <= 1e-10 A_abs + 1e-13 max(A_abs) with A_abs the same assembly of |J| and |r|, entries with A_abs = 0 exactly 0, J^T r to
1e-10 of its largest entry, the objective to 1e-12 relative, the valid SAMPLE count exact and untouched by the term.
Shapes: 40 nodes, 300 samples, 1 .. 300 landmarks.  Each test prints what it achieved (-s).
"""
import json
import os

import numpy as np
import pytest
import torch

import landmark_np as LN
from oracle import gn_np as G
from oracle import oracle_np as O
from dynamicfusion_body_amd import _lib, scene, solve
from dynamicfusion_body_amd.device import current_stream_ptr

pytestmark = pytest.mark.gpu

IDENT = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
LW = 1.03 * G.twist_exp_dq(np.array([0.01, -0.02, 0.015, 0.3, -0.2, 0.1]))          # a global warp with |r_lw| = 1.03
RW = 0.7
N_NODES, N_SAMPLES = 40, 300


def unit_normals(S, rng):
    n = rng.standard_normal((S, 3))
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def graph(rng, K):
    npos = rng.uniform(0, 30, size=(N_NODES, 3))
    nw = rng.uniform(8, 14, size=N_NODES)
    tw = rng.standard_normal((N_NODES, 6)) * np.array([0.02, 0.02, 0.02, 0.3, 0.3, 0.3])
    return npos, nw, G.apply_twists(np.tile(IDENT, (N_NODES, 1)), tw)


def make_solver(K, rng, sample_box=(0, 30)):
    """A solver with its graph, 300 samples (60 % valid) and correspondences; returns (solver, node_pos, node_w)."""
    npos, nw, dq = graph(rng, K)
    node_nbr, _ = solve.sample_knn(npos, npos, nw, K)
    sv = solve.WarpSolver(knn=K, pcg_iters=5, distributed=False)
    sv.set_graph(npos, dq, nw, node_nbr=node_nbr)
    pts = rng.uniform(sample_box[0], sample_box[1], size=(N_SAMPLES, 3))
    sv.set_samples(pts, unit_normals(N_SAMPLES, rng))
    sv.set_correspondences(pts + 0.3 * rng.standard_normal((N_SAMPLES, 3)), rng.random(N_SAMPLES) >= 0.4)
    return sv, npos, nw


def landmark_set(L, rng, mode, box=(0, 30)):
    """(pos, target, valid, conf) of L landmarks in the caller's order; beyond L = 2 one is switched off by valid, one by conf = 0
    and one has a NaN target."""
    if mode == "one_tuple":                                           # a tight cluster: one node tuple, a run cut by the tiles
        pos = np.array([11.0, 13.0, 12.0]) + 0.01 * rng.standard_normal((L, 3))
    else:
        pos = rng.uniform(box[0], box[1], size=(L, 3))
    target = pos + 0.6 * rng.standard_normal((L, 3))
    valid = np.ones(L, dtype=np.uint8)
    conf = rng.uniform(0.5, 2.0, size=L)
    if L > 2:
        valid[rng.integers(0, L, size=max(1, L // 10))] = 0
        conf[rng.integers(0, L, size=max(1, L // 10))] = 0.0
        target[int(rng.integers(0, L)), 1] = np.nan
    return pos, target, valid, conf


def host_landmarks(sv):
    """The solver's landmarks as it holds them (sorted by node tuple), numpy: (pos, target, nbr, weights, valid, conf)."""
    lm = sv._lm
    f = lambda t: None if t is None else t.cpu().numpy()
    return f(lm["pos"]), f(lm["target"]), f(lm["nbr"]).astype(np.int64), f(lm["wts"]), f(lm["valid"]), f(lm["conf"])


def reference(sv, npos, nw, huber_s, weight, huber_l, max_dist):
    """The restatement's dense system of the solver's state: (A, A_abs, b, objective, valid samples, active landmarks (sorted))."""
    dq = sv.node_dq.cpu().numpy()
    pos, nrm, nbr = sv.spos.cpu().numpy(), sv.snrm.cpu().numpy(), sv.snbr.cpu().numpy().astype(np.int64)
    corr, valid = sv.corr.cpu().numpy(), sv.valid.cpu().numpy().astype(bool)
    node_nbr = sv.node_nbr.cpu().numpy().astype(np.int64)
    A, Aa, b, c = LN.dense_data_and_reg(dq, pos, nrm, corr, valid, nbr, node_nbr, npos, nw, LW, RW, huber_s)
    active = None
    if sv._lm is not None and sv._lm["L"] > 0 and weight != 0.0:
        lp, lt, lnbr, lw_, lv, lc = host_landmarks(sv)
        rows = LN.landmark_rows(dq, lp, lt, lnbr, lw_, LW, weight=weight, conf=lc, valid=lv, huber_delta=huber_l, max_dist=max_dist)
        A1, Aa1, b1, c1 = LN.dense_term(len(dq), rows, lnbr)
        A, Aa, b, c, active = A + A1, Aa + Aa1, b + b1, c + c1, rows["active"]
    return A, Aa, b, c, int(valid.sum()), active


def check_system(sv, ref, tag):
    """The solver's last build (+ term) against `reference`'s: returns the largest entrywise |A - A_o| / bound."""
    A_o, A_abs, b_o, cost_o, cnt_o, active = ref
    A, b = sv.dense_normal_equations()
    cost, cnt = sv.cost()
    assert cnt == cnt_o, (tag, cnt, cnt_o)                                    # the term leaves the sample count alone
    assert abs(cost - cost_o) <= 1e-12 * cost_o, (tag, cost, cost_o)
    assert np.abs(b - b_o).max() <= 1e-10 * np.abs(b_o).max(), (tag, np.abs(b - b_o).max(), np.abs(b_o).max())
    assert (A[A_abs == 0.0] == 0.0).all(), (tag, "non-zero entry where no row contributes")
    ratio = np.abs(A - A_o) / (1e-10 * A_abs + 1e-13 * A_abs.max())
    worst = float(ratio.max())
    assert worst <= 1.0, (tag, worst, np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    if active is not None:
        assert np.array_equal(sv._lm["active"].cpu().numpy().astype(bool), active), (tag, "active_out")
    return worst


def settings(sv, npos, nw, rng):
    """A Huber delta that is beyond 40 % of the landmarks' |d| and a gate that drops 20 % of them."""
    lp, lt, lnbr, lw_, _, _ = host_landmarks(sv)
    rows = LN.landmark_rows(sv.node_dq.cpu().numpy(), lp, lt, lnbr, lw_, LW)
    n = np.linalg.norm(rows["d"], axis=1)
    n = n[np.isfinite(n)]
    # (a percentile can fall ON a landmark's |d|, for one landmark it always does; the factor moves both thresholds off the data, so
    # no landmark sits within rounding of the gate -- the exact boundary is tests/test_landmark_np.py's)
    return 1.000123 * float(np.percentile(n, 60)), 1.000123 * float(np.percentile(n, 80))


# ---------------------------------------------------------------- 1. the system against the restatement
@pytest.mark.parametrize("K,L", [(K, L) for L in (1, 127, 128, 129, 300) for K in (1, 3, 4, 8)] + [(K, 129) for K in (2, 5, 6, 7)])
def test_system_vs_restatement(K, L):
    """build + term at knn 1, 3, 4, 8 and landmark counts on both sides of the 128-landmark tile, and at every other knn with one
    full tile plus a one-landmark tile (every instance of the kernel runs): Huber and gate off and on,
    valid = 0, conf = 0 and a NaN target inactive, active_out exact -- in the solver's order and in the caller's --, the same bits
    twice, the term additive bit for bit, and the no-op forms (weight 0, no landmarks, n = 0) equal to the plain build."""
    rng = np.random.default_rng(1600 + 10 * K + L)
    sv, npos, nw = make_solver(K, rng)
    pos, target, valid, conf = landmark_set(L, rng, "random")
    sv.set_landmarks(pos, target, conf=conf, valid=valid)         # (before the first build: the pattern holds their node pairs from the start)
    assert sv.landmark_weight == 0.0
    sv.build(LW, RW, 0.5)
    plain = sv.system.clone()                                     # weight 0: the plain build (its restatement: no term)
    check_system(sv, reference(sv, npos, nw, 0.5, 0.0, 0.0, 0.0), (K, L, "weight 0"))
    hub, gate = settings(sv, npos, nw, rng)
    worst = 0.0
    for weight, huber_l, max_dist in ((1.0, 0.0, 0.0), (2.5, hub, 0.0), (1.0, 0.0, gate), (0.5, hub, gate)):
        sv.landmark_weight, sv.landmark_huber, sv.landmark_max_dist = weight, huber_l, max_dist
        sv.build(LW, RW, 0.5)
        ref = reference(sv, npos, nw, 0.5, weight, huber_l, max_dist)
        worst = max(worst, check_system(sv, ref, (K, L, weight, huber_l, max_dist)))
        s1 = sv.system.clone()
        a1 = sv._lm["active"].clone()
        sv.build(LW, RW, 0.5)
        assert torch.equal(s1, sv.system) and torch.equal(a1, sv._lm["active"]), "two runs differ"
        # additivity: after = before + (the term added to a zeroed system)
        sv.system.zero_()
        sv._add_landmarks(LW, upper=False)
        assert torch.equal(s1, plain + sv.system), (K, L, "the term is not additive bit for bit")
        if max_dist == 0.0 and L > 2:
            # active_out in the caller's order: exactly the valid, confident landmarks with a finite target
            expect = (valid != 0) & (conf > 0) & np.isfinite(target).all(axis=1)
            assert np.array_equal(sv.landmark_active().cpu().numpy().astype(bool), expect)
            assert 0 < expect.sum() < L
        if max_dist > 0.0 and L >= 127:
            act = sv._lm["active"].cpu().numpy()
            assert 0.5 * L < act.sum() < 0.85 * L                           # the gate dropped some and kept most
    # the no-op forms: weight 0 again, no landmarks, n = 0
    sv.landmark_weight = 0.0
    sv.build(LW, RW, 0.5)
    assert torch.equal(sv.system, plain)
    sv.landmark_weight = 1.0
    sv.clear_landmarks()
    sv.build(LW, RW, 0.5)
    assert torch.equal(sv.system, plain)
    sv.set_landmarks(np.zeros((0, 3)), np.zeros((0, 3)))
    sv.build(LW, RW, 0.5)
    assert torch.equal(sv.system, plain)
    print("K=%d L=%d: largest |A - A_o| / bound %.3g" % (K, L, worst))


# ---------------------------------------------------------------- 2. tuple structure: one run cut by tiles, all distinct, a growing pattern
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_one_tuple_for_all_landmarks(K):
    """300 landmarks in one node tuple: one run, cut into three scratch rows by the tiles -- and a tile's hundred active rows of one
    run into passes of kTile / 3 landmarks, the run carried over their boundaries, in every instance of the kernel."""
    rng = np.random.default_rng(1700 + K)
    sv, npos, nw = make_solver(K, rng)
    pos, target, valid, conf = landmark_set(300, rng, "one_tuple")
    sv.set_landmarks(pos, target, conf=conf, valid=valid)
    sv.landmark_weight = 1.0
    sv.build(LW, RW, 0.0)
    assert sv._lm["plan"]["n_rows"] == 3 and len(torch.unique(sv._lm["nbr"], dim=0)) == 1
    w = check_system(sv, reference(sv, npos, nw, 0.0, 1.0, 0.0, 0.0), (K, "one tuple"))
    print("K=%d one tuple: %.3g" % (K, w))


@pytest.mark.parametrize("plan", ["device", "torch"])
@pytest.mark.parametrize("K", [3, 4, 8])
def test_all_tuples_distinct(K, plan):
    """129 landmarks with a node table of their own, every tuple different: 129 runs of one landmark over two tiles.  plan =
    "torch": the plan built from torch ops (what node counts too large for packed tuple keys take)."""
    rng = np.random.default_rng(1800 + K)
    if plan == "torch":
        _lib.set_option("py_plan_torch", 1)
    sv, npos, nw = make_solver(K, rng)
    L = 129
    tuples = set()
    while len(tuples) < L:
        tuples.add(tuple(rng.choice(N_NODES, size=K, replace=False).tolist()))
    nbr = np.array(sorted(tuples), dtype=np.int32)[rng.permutation(L)]
    pos = npos[nbr].mean(axis=1) + rng.standard_normal((L, 3))
    target = pos + 0.5 * rng.standard_normal((L, 3))
    sv.set_landmarks(pos, target, nbr=nbr)
    sv.landmark_weight = 1.5
    sv.build(LW, RW, 0.0)
    assert sv._lm["plan"]["n_rows"] == L
    w = check_system(sv, reference(sv, npos, nw, 0.0, 1.5, 0.0, 0.0), (K, "distinct", plan))
    print("K=%d distinct tuples (%s plan): %.3g" % (K, plan, w))


@pytest.mark.parametrize("first", ["samples", "landmarks"])
@pytest.mark.parametrize("K", [1, 4])
def test_landmark_tuples_no_sample_has(K, first):
    """Samples in one half of the graph, landmarks in the other: the pattern must grow to hold the landmarks' node pairs, whether
    it was built before the landmarks came (the "still covered?" path) or with them."""
    rng = np.random.default_rng(1900 + K)
    sv, npos, nw = make_solver(K, rng, sample_box=(0, 12))
    if first == "samples":
        sv.build(LW, RW, 0.0)
        blocks_before = sv.B
    pos, target, valid, conf = landmark_set(200, rng, "random", box=(18, 30))
    sv.set_landmarks(pos, target, conf=conf, valid=valid)
    sv.landmark_weight = 1.0
    sv.build(LW, RW, 0.0)
    if first == "samples" and K > 1:
        assert sv.B > blocks_before
    assert not np.isin(np.unique(sv._lm["nbr"].cpu().numpy()), np.unique(sv.snbr.cpu().numpy())).all()
    w = check_system(sv, reference(sv, npos, nw, 0.0, 1.0, 0.0, 0.0), (K, "grow", first))
    # new targets, no replanning: the plan object stays, the system follows
    plan = sv._lm["plan"]
    sv.set_landmark_targets(target + 0.1, valid=valid, conf=conf)
    sv.build(LW, RW, 0.0)
    assert sv._lm["plan"] is plan
    w = max(w, check_system(sv, reference(sv, npos, nw, 0.0, 1.0, 0.0, 0.0), (K, "grow", first, "new targets")))
    print("K=%d pattern grown (%s first): %.3g" % (K, first, w))


# ---------------------------------------------------------------- 3. the one-call solve
def per_call_sequence(sv, prob_args, term_on, frame, sp, n_global, n_iters):
    """dfh_gn_solve_landmarks' schedule as separate library calls on the same problem."""
    lib, st = sv.lib, current_stream_ptr()
    for it in range(n_global + n_iters):
        prob = sv._problem(*prob_args)
        _lib.check(lib.dfh_gn_build(prob, frame, st), "dfh_gn_build")
        if term_on:
            _lib.check(lib.dfh_gn_add_landmarks(prob, sv._landmark_term(), st), "dfh_gn_add_landmarks")
        if it < n_global:
            sv.global_step(sp.global_lm)
        else:
            sv.solve_update(sp.lm_abs, sp.lm_rel)


@pytest.mark.parametrize("K", [3, 4])
def test_one_call_solve_without_a_frame(K):
    """dfh_gn_solve_landmarks(frame = NULL): two rigid-mode steps and four node iterations on the problem's corr / valid leave the
    node DQs bit for bit those of the per-call sequence; the term moves them (they differ from the solve without landmarks)."""
    rng = np.random.default_rng(2000 + K)
    sv, npos, nw = make_solver(K, rng)
    pos, target, valid, conf = landmark_set(300, rng, "random")
    sv.set_landmarks(pos, target, conf=conf, valid=valid)
    sv.landmark_weight, sv.landmark_huber = 1.0, 0.8
    sv.build(LW, RW, 0.5)
    dq0 = sv.node_dq.clone()
    args = (LW, RW, 0.5)
    out = {}
    for mode in ("one_call", "per_call", "no_landmarks"):
        sv.node_dq.copy_(dq0)
        sp = sv._solve_params(1e-3, 1e-2, 4, 2, 0.1, False)
        if mode == "one_call":
            _lib.check(sv.lib.dfh_gn_solve_landmarks(sv._problem(*args), None, sv._landmark_term(), sp, current_stream_ptr()),
                       "dfh_gn_solve_landmarks")
        else:
            per_call_sequence(sv, args, mode == "per_call", None, sp, 2, 4)
        out[mode] = sv.node_dq.clone()
    sv.check_status()
    assert torch.isfinite(out["one_call"]).all()
    assert torch.equal(out["one_call"], out["per_call"])
    assert not torch.equal(out["one_call"], out["no_landmarks"])


# ---------------------------------------------------------------- 4. recovery: what the term is for
@pytest.fixture(scope="module")
def record():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "landmark_recovery.json")) as f:
        return json.load(f)


def device_recovery(s, weight, pcg_iters):
    sv = solve.WarpSolver(knn=s["knn"], pcg_iters=pcg_iters, distributed=False)
    sv.set_graph(s["node_pos"], np.tile(IDENT, (s["N"], 1)), s["node_w"], node_nbr=s["node_nbr"])
    sv.set_samples(s["pos"], s["nrm"], nbr=s["nbr"])
    sv.set_correspondences(s["corr"])
    sv.set_landmarks(s["lpos"], s["ltarget"], nbr=s["lnbr"])
    sv.landmark_weight = weight
    costs = []
    for _ in range(s["iters"]):                                         # the device loop: build -> term -> solve_update
        sv.build(s["lw"], s["rw"])
        costs.append(sv.cost()[0])
        sv.solve_update(s["lm_abs"], s["lm_rel"])
    sv.check_status()
    return costs, sv.node_dq.cpu().numpy()


@pytest.mark.parametrize("kind", ["uniform", "ramped"])
def test_recovery_of_a_slide_inside_the_surface(record, kind):
    """The cylinder sliding along its axis (tests/landmark_np.py: recovery_scene).  Plane rows alone: no node moves.  With 200
    landmarks at weight 1 the held-out tangential error falls below half, the cost never rises, and the device's error agrees
    with the restatement's to 1e-5 (the node-DQ bar of the one-call oracle test): with the PCG iteration count at which the
    restatement's truncated loop meets its exact loop to 1e-6 (in the record) against the exact loop, and at the shipped 10
    iterations against the restatement's truncated loop."""
    s, rec = LN.recovery_scene(kind), record[kind]
    before = LN.heldout_rms(s, np.tile(IDENT, (s["N"], 1)))
    assert abs(before - rec["rms_before"]) <= 1e-12
    costs, dq = device_recovery(s, 0.0, 10)
    plane = LN.heldout_rms(s, dq)
    assert abs(plane - before) < 0.01 * before
    p = rec["pcg_iters_converged"]
    costs, dq = device_recovery(s, 1.0, p)
    rms = LN.heldout_rms(s, dq)
    print("%s: held-out RMS %.6f -> plane rows %.6f, landmarks %.6f (restatement %.6f), cost %.4f -> %.4f"
          % (kind, before, plane, rms, rec["weight_1"]["rms_after"], costs[0], costs[-1]))
    assert rms < 0.5 * before
    assert all(b <= a * (1 + 1e-12) for a, b in zip(costs, costs[1:]))
    assert abs(costs[0] - rec["weight_1"]["cost_first"]) <= 1e-12 * rec["weight_1"]["cost_first"]
    assert abs(rms - rec["weight_1"]["rms_after"]) <= 1e-5
    _, dq10 = device_recovery(s, 1.0, 10)
    rms10 = LN.heldout_rms(s, dq10)
    print("%s: at 10 PCG iterations %.6f (restatement's truncated loop %.6f)" % (kind, rms10, rec["rms_after_pcg10"]))
    assert abs(rms10 - rec["rms_after_pcg10"]) <= 1e-5


# ---------------------------------------------------------------- 5. the frame loop
def test_frame_loop_with_landmarks():
    """SlabFrame.step on a 32^3 scene with landmarks set: the one-call solve (dfh_gn_solve_landmarks with the frame, rigid-mode steps
    from the built system) leaves the node DQs of the per-call sequence bit for bit, the landmarks survive the sample refresh and a
    new graph, and they pull: the field differs from the frame solved without them."""
    from dynamicfusion_body_amd.pipeline import SlabFrame
    R, N = 32, 24
    H, W, fx, cx, cy = scene.CAMERAS["C1"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    lw = scene.view_extrinsic(0.0)
    d0 = torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda()
    d1 = torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0,
                                             sphere_offset=np.array([0.3, -0.2, 0.1]) * scale)).cuda()

    def frame():
        sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=2.0, distributed=False)
        sf.integrate(d0, lw)
        assert sf.refresh_samples() > 300
        return sf

    def landmarks_of(sf):
        pts = sf.fs.solver.spos[::7][:60].clone()
        return pts, pts + torch.tensor([0.3, -0.2, 0.1], dtype=torch.float64, device="cuda")

    fields = {}
    for mode in ("none", "one_call", "per_call"):
        sf = frame()
        if mode != "none":
            pts, tgt = landmarks_of(sf)
            sf.set_landmarks(pts, tgt, weight=2.0, huber=1.0, max_dist=3.0)
        if mode == "per_call":
            _lib.set_option("py_gn_no_fused_iter", 1)
        sf.step(d1, lw, gn_iters=4, relax=1.0)
        _lib.set_option("py_gn_no_fused_iter", None)
        fields[mode] = sf.fs.solver.node_dq.clone()
        assert torch.isfinite(fields[mode]).all()
        if mode == "one_call":
            kept = sf
    assert torch.equal(fields["one_call"], fields["per_call"])
    assert not torch.equal(fields["one_call"], fields["none"])
    sv = kept.fs.solver
    assert sv._lm is not None and sv._lm["L"] == 60 and int(sv.landmark_active().sum()) > 30      # survived the sample refresh
    # a new graph: the landmarks are handed to the solver again, with node tuples of the new graph
    n_nodes = kept.construct_graph(4.0)
    sv = kept.fs.solver
    assert sv._lm is not None and sv._lm["L"] == 60 and int(sv._lm["nbr"].max()) < n_nodes
    kept.step(d1, lw, gn_iters=2)
    assert torch.isfinite(sv.node_dq).all() and int(sv.landmark_active().sum()) > 30
    kept.clear_landmarks()
    assert sv._lm is None and not kept.fs.landmarks_active()


def test_fusion_hands_its_correspondences_over_as_landmarks():
    """Fusion.landmark_weight > 0: solve() gives (_vertices, _correspondences) to its WarpSolver as landmarks beside the plane rows.
    On the sliding cylinder the plane rows see nothing -- the field stays the identity -- and with the weight the nodes move along z."""
    from dynamicfusion_body_amd import Fusion
    s = LN.recovery_scene("uniform")
    N = s["N"]
    verts = np.concatenate([s["node_pos"], s["pos"]])                 # node i is anchored at vertex i
    nrm = np.concatenate([s["node_pos"] * np.array([1.0 / 6.0, 1.0 / 6.0, 0.0]), s["nrm"]])
    nbr = O.knn_bruteforce(verts, s["node_pos"], s["knn"])
    moved = {}
    for weight in (0.0, 1.0):
        fu = Fusion(np.zeros((4, 4, 4)), 1.0, knn=s["knn"], write_warpfield=False)
        assert fu.landmark_weight == 0.0                              # the default: today's solve
        fu._nodes = [(i, s["node_pos"][i], IDENT.copy(), float(s["node_w"][i])) for i in range(N)]
        fu._vertices, fu._normals, fu._correspondences = verts, nrm, LN.slide(verts, "uniform")
        fu._neighbor_look_up = [row for row in nbr]
        fu._lw = IDENT.copy()
        fu.landmark_weight = weight
        fu.solve(precompute_lw=False, regularization_weight=s["rw"], iterations=5)
        dq = np.stack([n[2] for n in fu._nodes])
        assert np.isfinite(dq).all()
        moved[weight] = float(2.0 * dq[:, 7].mean())
    print("mean node translation along z: plane rows %.3g, with landmarks %.3g (the slide: 0.2)" % (moved[0.0], moved[1.0]))
    assert abs(moved[0.0]) < 1e-9 and 0.1 < moved[1.0] < 0.3, moved
