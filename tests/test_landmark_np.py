"""CPU: the restatement of the landmark term (tests/landmark_np.py) -- its Jacobian against central differences of the rounding-free
warp, the vector Huber loss and the distance gate at their thresholds, and the recovery scene the device loop is compared with
(tests/test_gpu_landmarks.py), recorded in tests/golden/landmark_recovery.json.

    python tests/test_landmark_np.py --write      rewrites the record
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

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "landmark_recovery.json")
IDENT = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])


def small_problem(seed, identity=False, N=7, L=12, k=3):
    rng = np.random.default_rng(seed)
    node_pos = rng.uniform(0, 10, size=(N, 3))
    node_w = rng.uniform(3, 6, size=N)
    tw = rng.standard_normal((N, 6)) * np.array([0.3, 0.3, 0.3, 1.0, 1.0, 1.0])
    dqs = np.tile(IDENT, (N, 1)) if identity else G.apply_twists(np.tile(IDENT, (N, 1)), tw)
    lw = IDENT.copy() if identity else 1.03 * G.twist_exp_dq(np.array([0.2, -0.1, 0.15, 0.3, -0.2, 0.1]))
    pos = rng.uniform(0, 10, size=(L, 3))
    nbr = O.knn_bruteforce(pos, node_pos, k)
    w = G.blend_weights(pos, node_pos[nbr], node_w[nbr])
    target = pos + rng.standard_normal((L, 3))
    return dqs, lw, pos, nbr, w, target


@pytest.mark.parametrize("identity", [False, True])
def test_analytic_jacobian_vs_smooth_fd(identity):
    """J_a = d x'_a / d xi against central differences (h = 1e-5) of the warp without the float32 roundings, at random DQs with a
    non-unit lw and at the identity: |J - fd| <= 1e-7 max(1, |fd|), the bar the data rows' Jacobian meets in test_gn_oracle.py."""
    dqs, lw, pos, nbr, w, target = small_problem(5, identity)
    N, L, k = len(dqs), len(pos), nbr.shape[1]
    rows = LN.landmark_rows(dqs, pos, target, nbr, w, lw, round_f32=False)
    assert rows["active"].all()
    J = np.zeros((L, 3, N, 6))
    for j in range(k):
        J[np.arange(L), :, nbr[:, j], :] += rows["J"][:, :, j, :]
    h, worst = 1e-5, 0.0
    for a in range(N):
        for i in range(6):
            xi = np.zeros((N, 6))
            xi[a, i] = h
            dp = LN.landmark_rows(G.apply_twists(dqs, xi), pos, target, nbr, w, lw, round_f32=False)["d"]
            dm = LN.landmark_rows(G.apply_twists(dqs, -xi), pos, target, nbr, w, lw, round_f32=False)["d"]
            fd = (dp - dm) / (2 * h)
            err = np.abs(J[:, :, a, i] - fd) / np.maximum(1.0, np.abs(fd))
            worst = max(worst, float(err.max()))
    print("identity=%s: worst |J - fd| / max(1, |fd|) = %.3g" % (identity, worst))
    assert worst <= 1e-7


def test_huber_objective_and_scale_around_delta():
    """At, just below and just above delta: quadratic up to and including |d| = delta, linear beyond; the two branches meet."""
    delta, s2 = 0.75, 1.7
    below, above = np.nextafter(delta, 0.0), np.nextafter(delta, 1.0)
    q = np.array([below * below, delta * delta, above * above, 4.0 * delta * delta])
    obj, sc = LN.huber(q, np.full(4, s2), delta)
    assert obj[0] == 0.5 * s2 * q[0] and sc[0] == np.sqrt(s2)
    assert obj[1] == 0.5 * s2 * q[1] and sc[1] == np.sqrt(s2)                  # q == delta^2 is NOT beyond
    if q[2] > delta * delta:
        n = np.sqrt(q[2])
        assert obj[2] == s2 * delta * (n - 0.5 * delta) and sc[2] == np.sqrt(s2) * np.sqrt(delta / n)
    assert obj[3] == s2 * delta * (2.0 * delta - 0.5 * delta) and sc[3] == np.sqrt(s2) * np.sqrt(0.5)
    assert abs(obj[2] - obj[1]) <= 1e-14 and abs(sc[2] - sc[1]) <= 1e-14     # continuous across delta
    # sc^2 q is the IRLS row energy: beyond delta it is s2 delta |d|
    assert abs(sc[3] ** 2 * q[3] - s2 * delta * 2.0 * delta) <= 1e-14
    obj0, sc0 = LN.huber(q, np.full(4, s2), 0.0)                               # delta = 0: plain least squares
    assert np.array_equal(obj0, 0.5 * s2 * q) and (sc0 == np.sqrt(s2)).all()


def test_gate_keeps_exactly_max_dist_and_drops_what_the_term_lists():
    """Identity warp and float32-exact points: x' = p exactly, d = (3, 4, 0), q = 25.  max_dist = 5 keeps the landmark, the
    next double below drops it; valid = 0, conf = 0, a negative conf, a NaN or infinite target are inactive; max_dist <= 0: no gate."""
    N, k = 4, 2
    node_pos = np.array([[0.0, 0, 0], [8, 0, 0], [0, 8, 0], [8, 8, 0]])
    dqs = np.tile(IDENT, (N, 1))
    pos = np.array([[1.0, 2, 3], [5, 6, 1], [2, 7, 4], [6, 1, 2], [3, 3, 3], [4, 4, 1]])
    nbr = O.knn_bruteforce(pos, node_pos, k)
    w = G.blend_weights(pos, node_pos[nbr], np.full((len(pos), k), 4.0))
    target = pos - np.array([3.0, 4.0, 0.0])
    rows = LN.landmark_rows(dqs, pos, target, nbr, w, IDENT, max_dist=5.0)
    assert np.array_equal(rows["d"], np.tile([3.0, 4.0, 0.0], (len(pos), 1)))
    assert rows["active"].all() and np.allclose(rows["obj"], 12.5)
    assert not LN.landmark_rows(dqs, pos, target, nbr, w, IDENT, max_dist=np.nextafter(5.0, 0.0))["active"].any()
    assert LN.landmark_rows(dqs, pos, target, nbr, w, IDENT, max_dist=0.0)["active"].all()
    assert LN.landmark_rows(dqs, pos, target, nbr, w, IDENT, max_dist=-1.0)["active"].all()
    t2 = target.copy()
    t2[3, 1] = np.nan
    t2[4, 0] = np.inf
    rows = LN.landmark_rows(dqs, pos, t2, nbr, w, IDENT, valid=[0, 1, 1, 1, 1, 1], conf=[1, 0, -2.0, 1, 1, 0.5])
    assert rows["active"].tolist() == [False, False, False, False, False, True]
    assert (rows["r"][:5] == 0).all() and (rows["J"][:5] == 0).all() and (rows["obj"][:5] == 0).all()
    assert rows["obj"][5] == 0.5 * 0.5 * 25.0
    assert not LN.landmark_rows(dqs, pos, target, nbr, w, IDENT, weight=0.0)["active"].any()


# ---------------------------------------------------------------- the recovery scene
PCG_LADDER = (10, 20, 40, 80, 160, 320)


def recovery_record():
    rec = {}
    for kind in ("uniform", "ramped"):
        s = LN.recovery_scene(kind)
        before = LN.heldout_rms(s, np.tile(IDENT, (s["N"], 1)))
        out = {"rms_before": before}
        for name, weight in (("plane_only", 0.0), ("weight_1", 1.0)):
            costs, dqs = LN.recovery_loop(s, weight)
            out[name] = {"cost_first": costs[0], "cost_last": costs[-1], "rms_after": LN.heldout_rms(s, dqs),
                         "monotone": bool(all(b <= a * (1 + 1e-12) for a, b in zip(costs, costs[1:])))}
        exact = out["weight_1"]["rms_after"]
        for p in PCG_LADDER:
            _, dqs = LN.recovery_loop(s, 1.0, pcg_iters=p)
            if abs(LN.heldout_rms(s, dqs) - exact) <= 1e-6:
                out["pcg_iters_converged"] = p
                break
        _, dqs = LN.recovery_loop(s, 1.0, pcg_iters=10)
        out["rms_after_pcg10"] = LN.heldout_rms(s, dqs)
        rec[kind] = out
    return rec


@pytest.fixture(scope="module")
def record():
    return recovery_record()


@pytest.mark.parametrize("kind", ["uniform", "ramped"])
def test_recovery_scene_conditions(record, kind):
    """What the scene must show for the term to mean anything: the plane rows alone leave the held-out tangential error where it
    was (less than 1 % change), 200 landmarks at weight 1 bring it below half in ten iterations, and the cost never rises."""
    r = record[kind]
    print(kind, json.dumps(r))
    assert abs(r["plane_only"]["rms_after"] - r["rms_before"]) < 0.01 * r["rms_before"]
    assert r["weight_1"]["rms_after"] < 0.5 * r["rms_before"]
    assert r["weight_1"]["monotone"] and r["plane_only"]["monotone"]
    assert "pcg_iters_converged" in r


@pytest.mark.parametrize("kind", ["uniform", "ramped"])
def test_recovery_scene_matches_its_record(record, kind):
    """tests/golden/landmark_recovery.json is this file's output (the GPU test reads its PCG iteration count)."""
    with open(RECORD) as f:
        gold = json.load(f)[kind]
    r = record[kind]
    assert gold["pcg_iters_converged"] == r["pcg_iters_converged"]
    for a, b in ((gold["rms_before"], r["rms_before"]), (gold["rms_after_pcg10"], r["rms_after_pcg10"])) + tuple(
            (gold[n][f], r[n][f]) for n in ("plane_only", "weight_1") for f in ("cost_first", "cost_last", "rms_after")):
        assert abs(a - b) <= 1e-7 * max(abs(a), 1e-3), (kind, a, b)


if __name__ == "__main__":
    rec = recovery_record()
    print(json.dumps(rec, indent=1))
    if "--write" in sys.argv:
        with open(RECORD, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
