"""CPU: the restatement of the photometric term (tests/photometric_np.py) -- its Jacobian against central differences of the
rounding-free chain warp -> projection -> bilinear intensity, every gate on a representable boundary, and the recovery scene the
device loop is compared with (tests/test_gpu_photometric.py), recorded in tests/golden/photometric_recovery.json.

    python tests/test_photometric_np.py --write      rewrites the record
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import gn_np as G          # noqa: E402
from oracle import oracle_np as O      # noqa: E402
import landmark_np as LN               # noqa: E402
import photometric_np as PN            # noqa: E402

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photometric_recovery.json")
IDENT = PN.IDENT


@pytest.mark.parametrize("n_views", [1, 3])
@pytest.mark.parametrize("identity", [False, True])
def test_analytic_jacobian_vs_smooth_fd(identity, n_views):
    """J = g . d x' / d xi against central differences (h = 1e-5) of I through the chain without the float32 roundings, the view
    held fixed, at random DQs with a non-unit lw and at the identity; samples drawn with fu, fv in [0.1, 0.9] so that the step stays
    inside one bilinear cell: |J - fd| <= 1e-7 max(1, |fd|), the landmark term's bar.  Measured worst: 1.0e-8 (random DQs, one
    view), 8.2e-9 (three views), 7.2e-9 and 5.6e-9 at the identity.  A sample over an empty depth pixel has no row and is left out."""
    f = PN.fixture(18 + n_views, 3, 24, n_views, identity=identity, cell_margin=0.1, band_sd=np.inf)
    dqs, lw, pos, nbr, w, fr = f["dqs"], f["lw"], f["pos"], f["nbr"], f["w"], f["frame"]
    N, L, k = f["N"], len(pos), f["knn"]
    rows = PN.photo_rows(dqs, pos, f["ref"], nbr, w, lw, fr, round_f32=False)
    act = rows["active"]                                                      # (a sample over an empty depth pixel has no row)
    assert act.sum() >= 16
    pos, nbr, w, L = pos[act], nbr[act], w[act], int(act.sum())
    rows = {k: (v[act] if isinstance(v, np.ndarray) and len(v) == len(act) else v) for k, v in rows.items()}
    fu, fv = rows["u"] - np.floor(rows["u"]), rows["v"] - np.floor(rows["v"])
    assert fu.min() >= 0.1 and fu.max() <= 0.9 and fv.min() >= 0.1 and fv.max() <= 0.9
    assert np.abs(rows["g"]).max() > 1.0                                      # the images have gradients to differentiate
    J = np.zeros((L, N, 6))
    for j in range(k):
        J[np.arange(L), nbr[:, j], :] += rows["J"][:, j, :]
    h, worst = 1e-5, 0.0
    for a in range(N):
        for i in range(6):
            xi = np.zeros((N, 6))
            xi[a, i] = h
            Ip = PN.intensity_smooth(G.apply_twists(dqs, xi), pos, nbr, w, lw, fr, rows["view"])
            Im = PN.intensity_smooth(G.apply_twists(dqs, -xi), pos, nbr, w, lw, fr, rows["view"])
            fd = (Ip - Im) / (2 * h)
            err = np.abs(J[:, a, i] - fd) / np.maximum(1.0, np.abs(fd))
            worst = max(worst, float(err.max()))
    print("identity=%s views=%d: worst |J - fd| / max(1, |fd|) = %.3g" % (identity, n_views, worst))
    assert worst <= 1e-7


def test_projection_is_exact_in_the_boundary_scene():
    """The boundary scene's premise: u = x + cx and v = y + cy exactly, I an integer at integer pixels, sd = depth - 16."""
    b, _ = PN.boundary_cases()
    pos = np.array([[-2.5, -1.5, 16.0], [7.5, 0.25, 16.0]])
    nbr = O.knn_bruteforce(pos, b["node_pos"], b["knn"])
    w = G.blend_weights(pos, b["node_pos"][nbr], b["node_w"][nbr])
    rows = PN.photo_rows(b["dqs"], pos, np.zeros(2), nbr, w, b["lw"], PN.boundary_frame(b, depth=16.5), band_sd=1.0)
    assert np.array_equal(rows["xp"], pos)
    assert rows["u"][0] == 5.0 and rows["v"][0] == 4.0 and rows["I"][0] == float(b["Y"][4, 5]) and rows["sd"][0] == 0.5
    assert rows["view"].tolist() == [0, -1]                                   # u = 15 = W - 1 is outside


def test_gates_on_representable_boundaries():
    """u = W - 1 against the largest double below it, fabs(sd) == band_sd, fabs(r) == max_diff with integer images, NaN ref,
    conf = 0, valid = 0, and two views with equal |sd| (index 0 wins): the flags and views photometric_np.boundary_cases lists."""
    b, cases = PN.boundary_cases()
    assert len(cases) >= 15
    for name, fr, pos, ref, valid, conf, kw, exp_act, exp_view in cases:
        nbr = O.knn_bruteforce(pos, b["node_pos"], b["knn"])
        w = G.blend_weights(pos, b["node_pos"][nbr], b["node_w"][nbr])
        rows = PN.photo_rows(b["dqs"], pos, ref, nbr, w, b["lw"], fr, valid=valid, conf=conf, **kw)
        assert rows["active"].tolist() == exp_act, name
        assert rows["view"].tolist() == exp_view, name
        off = ~rows["active"]
        assert (rows["r"][off] == 0).all() and (rows["J"][off] == 0).all() and (rows["obj"][off] == 0).all(), name
        assert (rows["resid"][off] == 0).all(), name
    # the tie really is a tie, and the winner's image is the one that is read
    name, fr, pos, ref, _, _, kw, _, _ = [c for c in cases if c[0] == "tie +-"][0]
    nbr = O.knn_bruteforce(pos, b["node_pos"], b["knn"])
    w = G.blend_weights(pos, b["node_pos"][nbr], b["node_w"][nbr])
    rows = PN.photo_rows(b["dqs"], pos, ref, nbr, w, b["lw"], fr, **kw)
    assert rows["sd"][0] == 0.25 and rows["resid"][0] == 0.0                  # view 0's image is Y, view 1's Y + 3
    name, fr, pos, ref, _, _, kw, _, _ = [c for c in cases if c[0] == "view 1 nearer"][0]
    rows = PN.photo_rows(b["dqs"], pos, ref, nbr, w, b["lw"], fr, **kw)
    assert rows["sd"][0] == 0.125 and rows["resid"][0] == 3.0


def test_huber_is_the_landmark_terms_with_q_r_squared():
    """Scalar Huber on |r|: at delta the row is still quadratic, beyond it obj = s2 delta (|r| - delta / 2), sc = sqrt(s2 delta / |r|)."""
    b, cases = PN.boundary_cases()
    _, fr, pos, ref, _, _, _, _, _ = [c for c in cases if c[0] == "|r| = max_diff"][0]               # r = 7
    nbr = O.knn_bruteforce(pos, b["node_pos"], b["knn"])
    w = G.blend_weights(pos, b["node_pos"][nbr], b["node_w"][nbr])
    at = PN.photo_rows(b["dqs"], pos, ref, nbr, w, b["lw"], fr, weight=2.0, huber_delta=7.0)
    assert at["obj"][0] == 0.5 * 2.0 * 49.0 and at["r"][0] == np.sqrt(2.0) * 7.0
    out = PN.photo_rows(b["dqs"], pos, ref, nbr, w, b["lw"], fr, weight=2.0, huber_delta=1.75)
    assert out["obj"][0] == 2.0 * 1.75 * (7.0 - 0.5 * 1.75) and out["r"][0] == np.sqrt(2.0) * np.sqrt(1.75 / 7.0) * 7.0


# ---------------------------------------------------------------- the recovery scene
PCG_LADDER = (10, 20, 40, 80, 160, 320)


def recovery_record():
    rec = {}
    for kind in ("uniform", "ramped"):
        s, fr = LN.recovery_scene(kind), PN.recovery_frame(kind)
        before = LN.heldout_rms(s, np.tile(IDENT, (s["N"], 1)))
        out = {"rms_before": before, "weight": PN.PHOTO_WEIGHT, "band_sd": PN.BAND_SD}
        for name, weight in (("plane_only", 0.0), ("photo", PN.PHOTO_WEIGHT)):
            costs, dqs, n_act = PN.recovery_loop(s, fr, weight)
            out[name] = {"cost_first": costs[0], "cost_last": costs[-1], "rms_after": LN.heldout_rms(s, dqs), "active_last": n_act}
        exact = out["photo"]["rms_after"]
        for p in PCG_LADDER:
            _, dqs, _ = PN.recovery_loop(s, fr, PN.PHOTO_WEIGHT, pcg_iters=p)
            if abs(LN.heldout_rms(s, dqs) - exact) <= 1e-6:
                out["pcg_iters_converged"] = p
                break
        _, dqs, _ = PN.recovery_loop(s, fr, PN.PHOTO_WEIGHT, pcg_iters=10)
        out["rms_after_pcg10"] = LN.heldout_rms(s, dqs)
        rec[kind] = out
    return rec


@pytest.fixture(scope="module")
def record():
    return recovery_record()


@pytest.mark.parametrize("kind", ["uniform", "ramped"])
def test_recovery_scene_conditions(record, kind):
    """The cylinder sliding along its own axis under a painted texture and three analytic cameras: the plane rows alone leave the
    held-out tangential RMS where it was (to 1e-12), the colour rows of the solve's own 1 500 samples at weight 1e-3 bring it below
    half in ten exact iterations, and the last cost lies below the first (the cost is NOT monotone: 8-bit quantisation and the
    bilinear kinks make it oscillate after the third iteration)."""
    r = record[kind]
    print(kind, json.dumps(r))
    assert abs(r["plane_only"]["rms_after"] - r["rms_before"]) <= 1e-12
    assert r["photo"]["rms_after"] < 0.5 * r["rms_before"]
    assert r["photo"]["cost_last"] < r["photo"]["cost_first"]
    assert r["photo"]["active_last"] >= 1400
    assert "pcg_iters_converged" in r


@pytest.mark.parametrize("kind", ["uniform", "ramped"])
def test_recovery_scene_matches_its_record(record, kind):
    """tests/golden/photometric_recovery.json is this file's output (the GPU test reads its PCG iteration count)."""
    with open(RECORD) as f:
        gold = json.load(f)[kind]
    r = record[kind]
    assert gold["pcg_iters_converged"] == r["pcg_iters_converged"]
    assert gold["photo"]["active_last"] == r["photo"]["active_last"]
    for a, b in ((gold["rms_before"], r["rms_before"]), (gold["rms_after_pcg10"], r["rms_after_pcg10"])) + tuple(
            (gold[n][f], r[n][f]) for n in ("plane_only", "photo") for f in ("cost_first", "cost_last", "rms_after")):
        assert abs(a - b) <= 1e-7 * max(abs(a), 1e-3), (kind, a, b)


if __name__ == "__main__":
    rec = recovery_record()
    print(json.dumps(rec, indent=1))
    if "--write" in sys.argv:
        with open(RECORD, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
