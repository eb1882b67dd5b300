"""GPU: the photometric term (csrc/dfh_photometric.hip: gn_photo_rows_kernel<K> + the data term's gather with accumulate) against
its restatement (tests/photometric_np.py), from the kernel up to SlabFrame.step.

The system of the term alone is compared, dense, with the restatement's under tests/test_gpu_landmarks.py's bars: per entry
|A - A_o| <= 1e-10 A_abs + 1e-13 max(A_abs) with A_abs the same assembly of |J| and |r|, entries with A_abs = 0 exactly 0, J^T r to
1e-10 of its largest entry, the objective to 1e-12 relative, the valid SAMPLE count untouched.  active_out and view_out must be EQUAL
and resid_out equal to 1e-12: the fixture generator (photometric_np.fixture) rejects, on the CPU, samples whose u, v, sd or r lie
within 1e-9 relative of a decision boundary, so equality is what the op-for-op chain owes.
Shapes: 12 nodes, images of 16 x 12, 1 and 3 views, 1 .. 300 samples.  Each test prints what it achieved (-s).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import landmark_np as LN
import photometric_np as PN
from oracle import gn_np as G
from oracle import oracle_np as O
from dynamicfusion_body_amd import _lib, solve
from dynamicfusion_body_amd.device import current_stream_ptr

pytestmark = pytest.mark.gpu

IDENT = PN.IDENT
RW = 0.7


def device_frame(fr):
    """A restatement frame on the device: (frame tuple for build(frame=...), colour tensors, build_associated's leading arguments)."""
    depth = [torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).cuda() for d in fr["depth"]]
    colors = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in fr["color"]]
    lws = [m.reshape(12) for m in fr["lw_cam"]]
    args = (depth, fr["K"].reshape(9), fr["Kinv"].reshape(9), lws, fr["scale"], fr["center"], fr["half"])
    return args, colors


def make_solver(f, pcg_iters=5, dqs=None):
    sv = solve.WarpSolver(knn=f["knn"], pcg_iters=pcg_iters, distributed=False)
    sv.set_graph(f["node_pos"], f["dqs"] if dqs is None else dqs, f["node_w"], node_nbr=f["node_nbr"])
    sv.set_samples(f["pos"], f["nrm"], nbr=f["nbr"], weights=f["w"])
    return sv


def term_alone(sv, lw, frame_args, colors):
    """The term's system assembled into zeros (the gather walks every block)."""
    if sv._pattern is None:
        sv._build_pattern()
    sv.system.zero_()
    sv._add_photometric(lw, sv._photo_frame(frame_args), colors, upper=False)


def reference(sv, f, lw, settings, valid, conf):
    """The restatement's rows and dense system of the solver's samples (in the solver's order)."""
    weight, huber, max_diff = settings
    ph = sv._ph
    g = lambda t: None if t is None else t.cpu().numpy()
    nbr = sv.snbr.cpu().numpy().astype(np.int64)
    rows = PN.photo_rows(sv.node_dq.cpu().numpy(), sv.spos.cpu().numpy(), g(ph["ref"]), nbr, sv.swts.cpu().numpy(), lw, f["frame"],
                         weight=weight, conf=g(ph["conf"]), valid=g(ph["valid"]), huber_delta=huber, max_diff=max_diff, band_sd=f["band_sd"])
    return rows, PN.dense_term(f["N"], rows, nbr)


def check_term(sv, rows, dense, tag):
    """The solver's system (the term alone) and outputs against the restatement's: returns the largest |A - A_o| / bound."""
    A_o, A_abs, b_o, cost_o = dense
    A, b = sv.dense_normal_equations()
    cost, cnt = sv.cost()
    assert cnt == 0, (tag, "the term touched the sample count", cnt)
    ph = sv._ph
    assert np.array_equal(ph["active"].cpu().numpy().astype(bool), rows["active"]), (tag, "active_out")
    assert np.array_equal(ph["view"].cpu().numpy().astype(np.int64), rows["view"]), (tag, "view_out")
    resid = ph["resid"].cpu().numpy()
    assert (resid[~rows["active"]] == 0.0).all(), (tag, "resid_out of an inactive sample")
    assert np.abs(resid - rows["resid"]).max() <= 1e-12 * max(1.0, np.abs(rows["resid"]).max()), (tag, "resid_out")
    if not rows["active"].any():
        assert cost == 0.0 and (A == 0.0).all() and (b == 0.0).all(), tag
        return 0.0
    assert abs(cost - cost_o) <= 1e-12 * cost_o, (tag, cost, cost_o)
    assert np.abs(b - b_o).max() <= 1e-10 * np.abs(b_o).max(), (tag, np.abs(b - b_o).max(), np.abs(b_o).max())
    assert (A[A_abs == 0.0] == 0.0).all(), (tag, "non-zero entry where no row contributes")
    ratio = np.abs(A - A_o) / (1e-10 * A_abs + 1e-13 * A_abs.max())
    worst = float(ratio.max())
    assert worst <= 1.0, (tag, worst, np.unravel_index(int(np.argmax(ratio)), ratio.shape))
    return worst


def thresholds(f, lw):
    """A Huber delta that is beyond 40 % of the samples' |r| and a max_diff that drops 20 % (moved off the data by a factor, so no
    sample sits within rounding of either: the exact boundaries are test_boundaries_on_the_device's)."""
    rows = PN.photo_rows(f["dqs"], f["pos"], f["ref"], f["nbr"], f["w"], lw, f["frame"], band_sd=f["band_sd"])
    r = np.abs(rows["resid"][rows["active"]])
    return 1.000123 * float(np.percentile(r, 60)), 1.000123 * float(np.percentile(r, 80))


# ---------------------------------------------------------------- 1. the system of the term alone against the restatement
@pytest.mark.parametrize("n_views", [1, 3])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 300])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6, 7, 8])
def test_term_vs_restatement(K, n, n_views):
    """Every knn and sample counts on both sides of the 128-sample tile, one and three views: Huber and the gate off and on,
    valid = 0, conf = 0 and a NaN reference inactive, active_out / view_out equal and resid_out to 1e-12 -- in the solver's order and
    in the caller's --, and the same bits twice."""
    f = PN.fixture(1800 + 100 * K + n + n_views, K, n, n_views, seen_only=(n == 1))
    rng = np.random.default_rng(K + n)
    lw = f["lw"]
    args, colors = device_frame(f["frame"])
    sv = make_solver(f)
    ref, valid, conf = f["ref"].copy(), np.ones(n, dtype=np.uint8), rng.uniform(0.5, 2.0, size=n)
    if n > 2:
        valid[rng.integers(0, n, size=max(1, n // 10))] = 0
        conf[rng.integers(0, n, size=max(1, n // 10))] = 0.0
        ref[int(rng.integers(0, n))] = np.nan
    sv.set_photometric(ref, valid=valid, conf=conf)
    sv.photo_band_sd = f["band_sd"]
    hub, gate = thresholds(f, lw) if n > 2 else (0.0, 0.0)
    worst = 0.0
    for settings in ((1.0, 0.0, 0.0), (2.5, hub, gate)):
        sv.photo_weight, sv.photo_huber, sv.photo_max_diff = settings
        term_alone(sv, lw, args, colors)
        rows, dense = reference(sv, f, lw, settings, valid, conf)
        worst = max(worst, check_term(sv, rows, dense, (K, n, n_views, settings)))
        s1, a1 = sv.system.clone(), sv._ph["active"].clone()
        term_alone(sv, lw, args, colors)
        assert torch.equal(s1, sv.system) and torch.equal(a1, sv._ph["active"]), "two runs differ"
        if n > 2:
            act = sv.photometric_active().cpu().numpy().astype(bool)           # the caller's order
            assert not act[valid == 0].any() and not act[conf == 0.0].any() and not act[np.isnan(ref)].any()
            assert act.sum() == rows["active"].sum()
            rc = sv.photometric_residuals().cpu().numpy()
            order = sv._order_index().cpu().numpy() if sv.order is not None else np.arange(n)
            assert np.array_equal(rc[order], sv._ph["resid"].cpu().numpy())
            if n >= 127:
                assert 0.15 * n < act.sum() < n, act.sum()                       # the depth gate and the flags dropped some, kept many
    if n_views == 3 and n >= 127:
        assert len(np.unique(sv._ph["view"].cpu().numpy())) >= 3                 # more than one view was chosen (and -1)
    print("K=%d n=%d views=%d: largest |A - A_o| / bound %.3g, %d active" % (K, n, n_views, worst, int(rows["active"].sum())))


@pytest.mark.parametrize("K", [1, 4, 8])
def test_one_tuple_for_all_samples(K):
    """300 samples in one node tuple: one run, cut into three scratch rows by the tiles, each a long accumulation on the matrix cores."""
    f = PN.fixture(1900 + K, K, 300, 3, one_tuple=True)
    args, colors = device_frame(f["frame"])
    sv = make_solver(f)
    sv.set_photometric(f["ref"])
    sv.photo_weight, sv.photo_band_sd = 1.0, f["band_sd"]
    term_alone(sv, f["lw"], args, colors)
    assert sv.n_rows == 3 and len(torch.unique(sv.snbr, dim=0)) == 1
    rows, dense = reference(sv, f, f["lw"], (1.0, 0.0, 0.0), None, None)
    assert rows["active"].sum() > 100
    print("K=%d one tuple: %.3g" % (K, check_term(sv, rows, dense, (K, "one tuple"))))


def test_float64_depth_maps():
    """dfh_gn_add_photometric reads depth maps of either dtype: the float64 copies of the float32 maps give the same bits."""
    f = PN.fixture(1950, 4, 200, 3)
    args, colors = device_frame(f["frame"])
    sv = make_solver(f)
    sv.set_photometric(f["ref"])
    sv.photo_weight, sv.photo_band_sd = 1.0, f["band_sd"]
    term_alone(sv, f["lw"], args, colors)
    s32 = sv.system.clone()
    args64 = ([d.double() for d in args[0]],) + args[1:]
    term_alone(sv, f["lw"], args64, colors)
    assert torch.equal(s32, sv.system) and float(s32.abs().max()) > 0.0


# ---------------------------------------------------------------- 2. the gates on representable boundaries
def test_boundaries_on_the_device():
    """photometric_np.boundary_cases on the device: u = W - 1 against the largest double below it, fabs(sd) == band_sd,
    fabs(r) == max_diff with integer images, NaN ref, conf = 0, valid = 0, two views with equal |sd| -- the same flags, the same
    views, and the residuals (integers here) exactly."""
    b, cases = PN.boundary_cases()
    node_nbr = O.knn_bruteforce(b["node_pos"], b["node_pos"], b["knn"])
    for name, fr, pos, ref, valid, conf, kw, exp_act, exp_view in cases:
        nbr = O.knn_bruteforce(pos, b["node_pos"], b["knn"])
        w = G.blend_weights(pos, b["node_pos"][nbr], b["node_w"][nbr])
        sv = solve.WarpSolver(knn=b["knn"], pcg_iters=2, distributed=False)
        sv.set_graph(b["node_pos"], b["dqs"], b["node_w"], node_nbr=node_nbr)
        sv.set_samples(pos, np.tile([0.0, 0.0, 1.0], (len(pos), 1)), nbr=nbr, weights=w)
        sv.set_photometric(ref, valid=valid, conf=conf)
        sv.photo_weight = 1.0
        sv.photo_band_sd = kw.get("band_sd", float("inf"))
        sv.photo_max_diff = kw.get("max_diff", 0.0)
        args, colors = device_frame(fr)
        term_alone(sv, b["lw"], args, colors)
        rows = PN.photo_rows(b["dqs"], pos, ref, nbr, w, b["lw"], fr, valid=valid, conf=conf, **kw)
        assert sv.photometric_active().cpu().numpy().astype(bool).tolist() == exp_act, name
        assert sv.photometric_views().cpu().numpy().tolist() == exp_view, name
        assert np.array_equal(sv.photometric_residuals().cpu().numpy(), rows["resid"]), name


# ---------------------------------------------------------------- 3. additive, bit for bit; the null cases
def solver_with_data(f, rng, pcg_iters=5):
    sv = make_solver(f, pcg_iters)
    n = len(f["pos"])
    sv.set_correspondences(f["pos"] + 0.3 * rng.standard_normal((n, 3)), rng.random(n) >= 0.4)
    return sv


@pytest.mark.parametrize("K", [3, 4, 8])
def test_term_is_additive_bit_for_bit(K):
    """build, then the term, equals build's system plus the term's system assembled into zeros; weight 0, no colours, a cleared
    term and n == 0 leave the build's system bitwise untouched."""
    f = PN.fixture(2000 + K, K, 300, 3)
    rng = np.random.default_rng(K)
    args, colors = device_frame(f["frame"])
    sv = solver_with_data(f, rng)
    sv.build(f["lw"], RW, 0.5)
    plain = sv.system.clone()
    sv.set_photometric(f["ref"])
    sv.photo_band_sd = f["band_sd"]
    sv.build(f["lw"], RW, 0.5, colors=colors, frame=args)                       # weight 0 (the default): the plain build
    assert sv.photo_weight == 0.0 and torch.equal(sv.system, plain)
    sv.photo_weight, sv.photo_huber = 1.5, 12.0
    sv.build(f["lw"], RW, 0.5)                                                  # no colours: the plain build
    assert torch.equal(sv.system, plain)
    sv.build(f["lw"], RW, 0.5, colors=colors, frame=args)
    s1 = sv.system.clone()
    assert not torch.equal(s1, plain)
    sv.build(f["lw"], RW, 0.5, colors=colors, frame=args)
    assert torch.equal(s1, sv.system), "two runs differ"
    term_alone(sv, f["lw"], args, colors)
    assert torch.equal(s1, plain + sv.system), (K, "the term is not additive bit for bit")
    assert sv.cost()[1] == 0
    # n == 0 through the library: DFH_OK, nothing launched, the system as it was
    sv.build(f["lw"], RW, 0.5)
    t = sv._photo_term(colors, sv._photo_frame(args))
    t.n = 0
    _lib.check(sv.lib.dfh_gn_add_photometric(sv._problem(f["lw"], upper=False), sv._frm, t, current_stream_ptr()), "dfh_gn_add_photometric")
    torch.cuda.synchronize()
    assert torch.equal(sv.system, plain)
    sv.clear_photometric()
    sv.build(f["lw"], RW, 0.5, colors=colors, frame=args)
    assert torch.equal(sv.system, plain)


def landmarks_for(f, rng, L=60):
    pos = rng.uniform(0.5, 9.5, size=(L, 3))
    return pos, pos + 0.4 * rng.standard_normal((L, 3))


@pytest.mark.parametrize("with_landmarks", [False, True])
@pytest.mark.parametrize("K", [3, 4])
def test_one_call_solve_equals_the_per_call_sequence(K, with_landmarks):
    """dfh_gn_solve_photometric (two rigid-mode steps, three node iterations, the depth term fused into the builds) leaves the node
    DQs bit for bit those of the per-call sequence build -> landmarks -> colour rows -> step, with and without landmarks beside
    it; the term moves them; and without colors= the DQs are those of a solver that never had the term set."""
    f = PN.fixture(2100 + K, K, 300, 3)
    rng = np.random.default_rng(K)
    args, colors = device_frame(f["frame"])
    lm = landmarks_for(f, rng) if with_landmarks else None
    out = {}
    for mode in ("one_call", "per_call", "no_colors", "never_set"):
        sv = make_solver(f, pcg_iters=5)
        if lm is not None:
            sv.set_landmarks(*lm)
            sv.landmark_weight = 1.0
        if mode != "never_set":
            sv.set_photometric(f["ref"])
            sv.photo_weight, sv.photo_huber, sv.photo_band_sd = 1e-3, 15.0, f["band_sd"]
        if mode == "per_call":
            _lib.set_option("py_gn_no_fused_iter", 1)
        kw = {"colors": colors} if mode in ("one_call", "per_call") else {}
        try:
            sv.iterate_associated(args[0], args[1], args[2], args[3], args[4], args[5], args[6], f["lw"], RW, max_dist=3.0, huber=0.5,
                                  lm_abs=1e-3, lm_rel=1e-2, n_iters=3, n_global=2, **kw)
        finally:
            _lib.set_option("py_gn_no_fused_iter", None)
        sv.check_status()
        out[mode] = sv.node_dq.clone()
        assert torch.isfinite(out[mode]).all()
        if mode == "one_call":
            assert int(sv.photometric_active().sum()) > 50
            assert int(sv.valid.sum()) > 20                                     # the depth term associated samples too
    assert torch.equal(out["one_call"], out["per_call"])
    assert torch.equal(out["no_colors"], out["never_set"])
    assert not torch.equal(out["one_call"], out["no_colors"])


def test_bad_arguments_are_refused_before_anything_is_launched():
    """Every DFH_E_BADARG case of include/dfusion_hip.h through _lib (tests/test_photometric_badargs.py's table, which needs no
    device), and on a real solver's structs: a refused call leaves the system bitwise as it was."""
    import math
    import test_photometric_badargs as B
    lib = _lib.load()
    for name in sorted(B.CALLS):
        B.test_photometric_calls_refuse_bad_arguments(lib, name)
    B.test_solve_photometric_refuses_what_the_solve_refuses(lib)
    f = PN.fixture(2200, 4, 129, 3)
    rng = np.random.default_rng(22)
    args, colors = device_frame(f["frame"])
    sv = solver_with_data(f, rng)
    sv.set_photometric(f["ref"])
    sv.photo_weight, sv.photo_band_sd = 1.0, f["band_sd"]
    sv.build(f["lw"], RW, 0.5)
    plain = sv.system.clone()
    frame = sv._photo_frame(args)
    t = sv._photo_term(colors, frame)
    prob, st = sv._problem(f["lw"], upper=False), current_stream_ptr()
    bad = {"band_sd": (0.0, -1.0, math.nan), "max_diff": (math.nan,), "weight": (-1.0, math.inf, math.nan), "huber_delta": (-1.0, math.nan),
           "n": (-1,), "n_rows": (0,), "color": (None,), "ref": (None,), "pos": (None,), "partial": (None,), "run_id": (None,)}
    for field, values in bad.items():
        keep = getattr(t, field)
        for v in values:
            setattr(t, field, v)
            assert lib.dfh_gn_add_photometric(prob, frame, t, st) == B.BADARG, (field, v)
            assert lib.dfh_gn_solve_photometric(prob, frame, None, t, sv._solve_params(1e-3, 1e-2, 1, 0, 0.1, False), st) == B.BADARG, (field, v)
        setattr(t, field, keep)
    assert lib.dfh_gn_add_photometric(prob, None, t, st) == B.BADARG
    hole = (ctypes.c_void_p * 3)(int(colors[0].data_ptr()), None, int(colors[2].data_ptr()))
    keep, t.color = t.color, ctypes.cast(hole, ctypes.c_void_p)
    assert lib.dfh_gn_add_photometric(prob, frame, t, st) == B.BADARG
    t.color = keep
    torch.cuda.synchronize()
    assert torch.equal(sv.system, plain)
    t.band_sd = math.inf                                                        # +inf is allowed: no depth gate beyond "has depth"
    assert lib.dfh_gn_add_photometric(prob, frame, t, st) == B.OK
    torch.cuda.synchronize()
    assert not torch.equal(sv.system, plain) and bool(torch.isfinite(sv.system).all())


# ---------------------------------------------------------------- 4. recovery: what the term is for
@pytest.fixture(scope="module")
def record():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photometric_recovery.json")) as f:
        return json.load(f)


def device_recovery(s, fr, weight, pcg_iters):
    sv = solve.WarpSolver(knn=s["knn"], pcg_iters=pcg_iters, distributed=False)
    sv.set_graph(s["node_pos"], np.tile(IDENT, (s["N"], 1)), s["node_w"], node_nbr=s["node_nbr"])
    wts = G.blend_weights(s["pos"], s["node_pos"][s["nbr"]], s["node_w"][s["nbr"]])
    sv.set_samples(s["pos"], s["nrm"], nbr=s["nbr"], weights=wts)
    sv.set_correspondences(s["corr"])
    sv.set_photometric(PN.texture(s["pos"]))
    sv.photo_weight, sv.photo_band_sd = weight, PN.BAND_SD
    args, colors = device_frame(fr)
    costs = []
    for _ in range(s["iters"]):                                         # the device loop: build -> term -> solve_update
        sv.build(s["lw"], s["rw"], colors=colors, frame=args)
        costs.append(sv.cost()[0])
        sv.solve_update(s["lm_abs"], s["lm_rel"])
    sv.check_status()
    return costs, sv.node_dq.cpu().numpy(), int(sv.photometric_active().sum()) if weight > 0.0 else 0


@pytest.mark.parametrize("kind", ["uniform", "ramped"])
def test_recovery_of_a_slide_inside_the_surface(record, kind):
    """The textured cylinder sliding along its axis under three analytic cameras (tests/photometric_np.py).  Plane rows alone: no
    node moves.  With the colour rows of the solve's own 1 500 samples at weight 1e-3 the held-out tangential error falls below half
    and the device's error agrees with the restatement's to 1e-5: with the PCG iteration count at which the restatement's truncated
    loop meets its exact loop to 1e-6 (in the record) against the exact loop, and at the shipped 10 iterations against the
    restatement's truncated loop.  The cost is not monotone (8-bit quantisation, bilinear kinks): only last < first is asserted."""
    s, fr, rec = LN.recovery_scene(kind), PN.recovery_frame(kind), record[kind]
    before = LN.heldout_rms(s, np.tile(IDENT, (s["N"], 1)))
    assert abs(before - rec["rms_before"]) <= 1e-12
    _, dq, _ = device_recovery(s, fr, 0.0, 10)
    plane = LN.heldout_rms(s, dq)
    assert abs(plane - before) <= 1e-12
    p = rec["pcg_iters_converged"]
    costs, dq, n_act = device_recovery(s, fr, rec["weight"], p)
    rms = LN.heldout_rms(s, dq)
    print("%s: held-out RMS %.6f -> plane rows %.6f, colour rows %.6f (restatement %.6f), cost %.4f -> %.4f, %d active"
          % (kind, before, plane, rms, rec["photo"]["rms_after"], costs[0], costs[-1], n_act))
    assert rms < 0.5 * before
    assert costs[-1] < costs[0]
    assert abs(costs[0] - rec["photo"]["cost_first"]) <= 1e-12 * rec["photo"]["cost_first"]
    assert n_act == rec["photo"]["active_last"]
    assert abs(rms - rec["photo"]["rms_after"]) <= 1e-5
    _, dq10, _ = device_recovery(s, fr, rec["weight"], 10)
    rms10 = LN.heldout_rms(s, dq10)
    print("%s: at 10 PCG iterations %.6f (restatement's truncated loop %.6f)" % (kind, rms10, rec["rms_after_pcg10"]))
    assert abs(rms10 - rec["rms_after_pcg10"]) <= 1e-5


# ---------------------------------------------------------------- 5. the frame loop
def test_frame_loop_with_the_photometric_term():
    """SlabFrame(color_band=..., photo_weight > 0) at 32^3 with tests/color_np.py's painted sphere, three step(colors=...): the term
    is active for a non-zero share of the samples from the second step on (the first has no colour volume to take references
    from), nothing is non-finite, and the same loop with photo_weight = 0 equals a SlabFrame built without the argument bit for bit."""
    import color_np as CN
    from dynamicfusion_body_amd import scene
    from dynamicfusion_body_amd.pipeline import SlabFrame
    R, N = 32, 24
    H, W, fx, cx, cy = scene.CAMERAS["C1"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    lws = [scene.view_extrinsic(a) for a in (0.0, 0.5)]
    frames = []
    for i in range(4):
        off = np.array([0.1, -0.05, 0.05]) * scale * i
        depth = [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, sphere_offset=off)).cuda() for lw in lws]
        frames.append((depth, [painted(CN, K, lw, d.cpu().numpy(), off) for lw, d in zip(lws, depth)]))

    def run(**kw):
        sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=2.0, distributed=False,
                       color_band=2.0, **kw)
        sf.integrate(frames[0][0][0], lws[0])
        assert sf.refresh_samples() > 300
        shares = []
        for depth, colors in frames[1:]:
            sf.step(depth, lws, gn_iters=3, colors=colors)
            sv = sf.fs.solver
            assert torch.isfinite(sv.node_dq).all()
            shares.append(0.0 if sf.photo_active is None else float(sf.photo_active.float().mean()))
        assert torch.isfinite(sf.T).all() and torch.isfinite(sf.C).all()
        return sf.fs.solver.node_dq.clone(), sf.T.clone(), sf.C.clone(), shares

    dq_on, T_on, C_on, shares = run(photo_weight=1e-3, photo_huber=20.0)
    print("share of samples with an active colour row, per step: %s" % shares)
    assert shares[-1] > 0.0
    dq_0, T_0, C_0, _ = run(photo_weight=0.0)
    dq_n, T_n, C_n, _ = run()
    assert torch.equal(dq_0, dq_n) and torch.equal(T_0, T_n) and torch.equal(C_0, C_n)
    assert not torch.equal(dq_on, dq_n)                                        # the term pulled


def painted(CN, K, lw, depth, off):
    """A colour image of the sphere painted with color_np.analytic_color (as color_np.recovery_scene paints it), the paint moving
    with the sphere: each pixel's back-projected world position, less the sphere's offset, looked up in the colour field."""
    H, W = depth.shape
    Kinv = np.linalg.inv(K)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z = -1.0 * depth.astype(np.float64)
    cam = (z[..., None] * np.stack([u, v, np.ones_like(u)], axis=-1)) @ Kinv.T
    world = (cam - lw[:, 3]) @ lw[:, :3]
    img = np.zeros((H, W, 3), dtype=np.uint8)
    img[z > 0] = np.clip(np.rint(CN.analytic_color(world[z > 0] - off)), 0, 255).astype(np.uint8)
    return img


def test_several_ranks_are_refused(monkeypatch):
    """Single rank only: SlabFrame(photo_weight > 0) in a group of two raises at construction, and says why; without the weight the
    same construction goes through."""
    from dynamicfusion_body_amd import dist as D, scene
    from dynamicfusion_body_amd.pipeline import SlabFrame
    R = 32
    H, W, fx, cx, cy = scene.CAMERAS["C1"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(24, R)
    monkeypatch.setattr(D, "world", lambda: (0, 2))
    with pytest.raises(ValueError, match="single-rank"):
        SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, color_band=2.0, photo_weight=1e-3, solve_mode="replicated")
    sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, color_band=2.0, solve_mode="replicated")
    assert sf.ws == 2 and sf.photo_weight == 0.0
    monkeypatch.undo()
    with pytest.raises(ValueError, match="color_band"):
        SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, photo_weight=1e-3, distributed=False)
