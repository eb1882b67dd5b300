"""CPU: the numpy restatement of K21 (tests/track_np.py) against independent statements of the same mathematics, the tracking
scene (tests/track_cases.py), the recorded recovery figures (tests/golden/track_recovery.json) and the product's host helpers.

Bars.  The Jacobian is compared with central differences of r at h = 1e-6 on pixels whose model pixel does not change under the
perturbation: r is O(1), so the difference quotient carries ~1e-16 / 1e-6 = 1e-10 of rounding and O(h^2) = 1e-12 of truncation;
1e-8 leaves two digits.  The solve is compared with numpy.linalg.solve at 1e-9 relative (a 6 x 6 system whose condition the test
prints).  The golden figures are re-derived for the bar's motion and must match to 1e-6 degree and 1e-8 m (libm's sin and cos
may differ by an ulp between machines; nineteen iterations of a contraction do not amplify that)."""
import json
import math
import os

import numpy as np
import pytest

import track_cases as TC
import track_np as TN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_recovery.json")
BAR_SIZE = "1"          # the motion of the qualitative bar: 4.5 degrees and 111 mm (chosen from the JSON, see the test)


@pytest.fixture(scope="module")
def frame():
    """The scene from the identity (model) and from a small motion (live), with the restatement's live normals."""
    lw = TC.motion(0.3)
    live, _ = TC.render(lw)
    md, mn = TC.render(TC.IDENT)
    (_, D, n), = TC.live_pyramid(live, 1)
    return D, n, md, mn, lw


def test_scene_has_no_continuous_symmetry(frame):
    """The six columns of J are linearly independent on the scene: the Gauss-Newton matrix of the aligned frame has no null
    direction (its smallest eigenvalue is not small against its largest for a scene of a wall and two spheres)."""
    D, n, md, mn, _ = frame
    rows = TN.icp_rows(md, mn, md, mn, TC.K, np.linalg.inv(TC.K), TC.IDENT, 0.0, 0.0, 0.0)
    s, _ = TN.icp_sums(rows)
    assert s[28] > 15000
    A = np.zeros((6, 6))
    for q, (i, j) in enumerate(TN.PAIRS):
        A[i, j] = A[j, i] = s[q]
    ev = np.linalg.eigvalsh(A)
    print("eigenvalues", ev)
    assert ev[0] > 1e-4 * ev[-1]
    assert abs(s[27]) < 1e-8 * s[28]                                   # identical maps under the identity: r is rounding only


def test_jacobian_against_central_differences(frame):
    D, n, md, mn, _ = frame
    Kinv = np.linalg.inv(TC.K)
    T0 = TN.apply_twist(np.array([0.01, -0.02, 0.015, 0.01, 0.02, -0.01]), TC.IDENT)
    base = TN.icp_rows(D, n, md, mn, TC.K, Kinv, T0, 0.0, 0.0, 0.0)
    h = 1e-6
    rng = np.random.default_rng(5)
    for trial in range(6):
        xi = np.zeros(6)
        xi[trial] = 1.0
        if trial >= 3:
            xi = rng.standard_normal(6)
        rp = TN.icp_rows(D, n, md, mn, TC.K, Kinv, TN.apply_twist(h * xi, T0), 0.0, 0.0, 0.0)
        rm = TN.icp_rows(D, n, md, mn, TC.K, Kinv, TN.apply_twist(-h * xi, T0), 0.0, 0.0, 0.0)
        # same model pixel on all three: J3..5 = the model normal, read at that pixel
        same = (base[..., 7] > 0) & (rp[..., 7] > 0) & (rm[..., 7] > 0) & np.all(rp[..., 3:6] == base[..., 3:6], axis=-1) & \
            np.all(rm[..., 3:6] == base[..., 3:6], axis=-1)
        # a wall pixel keeps its normal when the model pixel changes: the residual's model point must not have moved either
        fd = (rp[..., 6] - rm[..., 6]) / (2 * h)
        an = base[..., :6] @ xi
        err = np.abs(fd - an)[same]
        assert same.sum() > 10000
        # pixels whose model pixel changed (rint jumps) show an O(1) difference quotient: they are the few above the bar
        jumped = int((err > 1e-8).sum())
        print("direction", trial, "pixels", int(same.sum()), "median", float(np.median(err)), "jumped", jumped)
        assert np.median(err) < 1e-9
        assert jumped <= 0.002 * same.sum()


def test_huber_weight_and_gates(frame):
    D, n, md, mn, _ = frame
    Kinv = np.linalg.inv(TC.K)
    plain = TN.icp_rows(D, n, md, mn, TC.K, Kinv, TC.IDENT, 0.0, 0.0, 0.0)
    hub = TN.icp_rows(D, n, md, mn, TC.K, Kinv, TC.IDENT, 0.0, 0.0, 0.01)
    r = plain[..., 6]
    big = np.abs(r) > 0.01
    assert big.any() and (~big & (plain[..., 7] > 0)).any()
    assert np.array_equal(hub[..., 7][big], 0.01 / np.abs(r[big]))
    assert np.all(hub[..., 7][~big & (plain[..., 7] > 0)] == 1.0)
    gated = TN.icp_rows(D, n, md, mn, TC.K, Kinv, TC.IDENT, 0.02, 0.9, 0.0)
    assert 0 < (gated[..., 7] > 0).sum() < (plain[..., 7] > 0).sum()
    assert np.all(plain[..., 7][gated[..., 7] > 0] > 0)
    none = TN.icp_rows(D, None, md, mn, TC.K, Kinv, TC.IDENT, 0.0, 0.0, 0.0)
    assert (none[..., 7] > 0).sum() >= (plain[..., 7] > 0).sum()


def test_depth_halve_rule():
    nan, inf = np.nan, np.inf
    D = np.array([[-1.0, -1.1, 0.0, -2.0, -3.0],
                  [-1.2, -5.0, -2.0, -2.0, -3.0],
                  [-1.0, nan, -1.0, -1.25, 7.0],
                  [-inf, 2.0, -0.75, -1.5, 7.0]], np.float32)
    out = TN.depth_halve(D, 0.25)
    assert out.shape == (2, 2) and out.dtype == np.float32
    assert out[0, 0] == np.float32((np.float32(-1.0) + np.float32(-1.1) + np.float32(-1.2)) / np.float32(3))     # -5 jumps
    assert out[0, 1] == 0.0                                                                                        # anchor invalid
    assert out[1, 0] == np.float32(-1.0)                                                                           # only the anchor
    assert out[1, 1] == np.float32((np.float32(-1.0) + np.float32(-1.25) + np.float32(-0.75)) / np.float32(3))   # jump == max_jump
    assert TN.depth_halve(D.astype(np.float64), 0.25).tobytes() == out.tobytes()
    assert TN.depth_halve(np.full((3, 2), nan, np.float32), 1.0).tolist() == [[0.0]]


def test_level_intrinsics_keep_the_rays():
    """The ray through coarse pixel x is the ray through the fine coordinate 2x + 0.5, the centre of the pixels it averages."""
    K1 = TN.level_intrinsics(TC.K)
    for x, y in ((0, 0), (7, 3), (79, 59)):
        fine = np.linalg.inv(TC.K) @ np.array([2 * x + 0.5, 2 * y + 0.5, 1.0])
        coarse = np.linalg.inv(K1) @ np.array([x, y, 1.0])
        assert np.allclose(fine, coarse, rtol=0, atol=1e-13)
    from dynamicfusion_body_amd import tracking
    assert np.array_equal(tracking.level_intrinsics(TC.K), K1)
    assert np.array_equal(tracking.CameraTracker(TC.K).Ks[2], TN.level_intrinsics(K1))


def test_se3_exponential():
    rng = np.random.default_rng(2)
    for scale in (1e-6, 9e-5, 1.1e-4, 0.3, 2.0):
        xi = scale * rng.standard_normal(6)
        R, Vm, t = TN.se3_exp(xi)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1) < 1e-14
        # against the power series of the 4 x 4 matrix exponential
        M = np.zeros((4, 4))
        o = xi[:3]
        M[:3, :3] = [[0, -o[2], o[1]], [o[2], 0, -o[0]], [-o[1], o[0], 0]]
        M[:3, 3] = xi[3:]
        E, term = np.eye(4), np.eye(4)
        for k in range(1, 40):
            term = term @ M / k
            E = E + term
        assert np.allclose(R, E[:3, :3], atol=1e-13) and np.allclose(t, E[:3, 3], atol=1e-13)
    T = TN.apply_twist(np.array([0.1, 0.2, -0.1, 0.3, 0.1, 0.2]), TC.motion(1.0))
    assert np.allclose(TN.compose(TN.invert_rigid(T), T), TC.IDENT, atol=1e-15)


def test_solve_and_refusals(frame):
    D, n, md, mn, _ = frame
    rows = TN.icp_rows(D, n, md, mn, TC.K, np.linalg.inv(TC.K), TC.IDENT, 0.0, 0.0, 0.0)
    s, _ = TN.icp_sums(rows)
    A = np.zeros((6, 6))
    for q, (i, j) in enumerate(TN.PAIRS):
        A[i, j] = A[j, i] = s[q]
    Dm = A + 1e-3 * np.diag(np.diag(A))
    status, xi, T1 = TN.icp_solve(s, TC.IDENT, 1e-3, 6, math.inf, math.inf)
    print("condition", np.linalg.cond(Dm))
    assert status == 1 and np.allclose(xi, np.linalg.solve(Dm, -s[21:27]), rtol=1e-9, atol=0)
    assert np.array_equal(T1, TN.apply_twist(xi, TC.IDENT))
    for kw in (dict(min_count=int(s[28]) + 1), dict(max_rot=1e-6), dict(max_trans=1e-6)):
        args = dict(lm_rel=1e-3, min_count=6, max_rot=math.inf, max_trans=math.inf)
        args.update(kw)
        status, xi, T1 = TN.icp_solve(s, TC.IDENT, **args)
        assert status == 0 and not xi.any() and np.array_equal(T1, TC.IDENT)
    # a single plane under the identity without damping: translations in the plane are free, a pivot is not positive
    z = np.full((24, 32), -1.5, np.float32)
    nz = np.zeros((24, 32, 3), np.float32)
    nz[..., 2] = -1.0
    Kp = np.array([[30.0, 0, 15.5], [0, 30.0, 11.5], [0, 0, 1]])
    prow = TN.icp_rows(z, nz, z, nz, Kp, np.linalg.inv(Kp), TC.IDENT, 0.0, 0.0, 0.0)
    ps, _ = TN.icp_sums(prow)
    assert ps[28] == 24 * 32
    assert TN.icp_solve(ps, TC.IDENT, 0.0, 6, math.inf, math.inf)[0] == 0
    nan_s = s.copy()
    nan_s[0] = np.nan
    assert TN.icp_solve(nan_s, TC.IDENT, 1e-3, 6, math.inf, math.inf)[0] == 0


def test_refused_steps_repeat(frame):
    D, n, md, mn, _ = frame
    T, stats = TN.icp_track(D, n, md, mn, TC.K, np.linalg.inv(TC.K), TC.IDENT, 0.0, 0.0, 0.0, 1e-3, 3, max_rot=1e-9)
    assert np.array_equal(T, TC.IDENT) and not stats[:, 29].any()
    assert np.array_equal(stats[0], stats[1]) and np.array_equal(stats[1], stats[2])


@pytest.mark.parametrize("size", list(TC.PASS_SHAPES))
def test_pass_cases_reach_every_pass_of_the_rows_grid(size):
    """The maps of tests/test_gpu_track.py::test_rows_and_sums_past_the_first_pass really make a workgroup of icp_rows_kernel walk
    a second and a third tile.  Asserted on the restatement, per view: the tile count is of the class the shape was chosen for;
    every pass holds a row that adds to the sums (w > 0, r != 0) and a pixel without a row, and so do both tiles of most workgroups
    that take two (in view 0); the one-pixel-high last tile row of (257, 528) holds such a row too; and the sums of pass 0 ALONE
    lie more than 100 of the GPU test's bounds away in every one of the 28 entries (measured: 1.6e8 at the least), and differ in the
    count: a kernel that dropped the later passes (or reset its accumulator between them) cannot pass."""
    H, W = size
    tiles, passes = TC.PASS_SHAPES[size]
    assert TC.n_tiles(H, W) == tiles and -(-tiles // TC.ICP_GRID) == passes
    c = TC.pass_case(H, W)
    assert c["tile"].max() == tiles - 1 and np.array_equal(np.unique(c["tile"]), np.arange(tiles))
    p_of = c["tile"] // TC.ICP_GRID
    for v in range(2):
        rows = c["rows"][v]
        live = (rows[..., 7] > 0) & (rows[..., 6] != 0)
        for p in range(passes):
            assert live[p_of == p].any() and not (rows[..., 7] > 0)[p_of == p].all(), (v, p)
        assert (rows[..., 7] < 1.0)[live].sum() > 100                              # Huber weights take part
        if passes > 1 and v == 0:
            # most workgroups that take two tiles find such a row in BOTH (view 0's T is the identity: no pixel leaves the map), and
            # one that takes three in all three: an accumulator that forgot a tile on the way to the next loses something
            has = np.bincount(c["tile"][live], minlength=tiles) > 0
            two = [has[t] and has[t + TC.ICP_GRID] for t in range(tiles - TC.ICP_GRID)]
            three = [has[t] and has[t + TC.ICP_GRID] and has[t + 2 * TC.ICP_GRID] for t in range(max(0, tiles - 2 * TC.ICP_GRID))]
            print(size, "workgroups with a row in each of two tiles", sum(two), "of", len(two), "of three", sum(three), "of", len(three))
            assert sum(two) >= 0.8 * len(two) and (not three or sum(three) >= 1)
        if size == (257, 528):
            assert H % 16 == 1 and live[H - 1].any() and p_of[H - 1].min() == 2     # the last tile row: one pixel high, in the partial pass
        exact, mag = TN.icp_sums(rows)
        n = int(exact[28])
        print(size, "view", v, "rows", n, "of", H * W)
        assert n > 0.5 * H * W
        if passes > 1:
            first, _ = TN.icp_sums(np.where((p_of == 0)[..., None], rows, 0.0))
            assert first[28] < n
            miss = np.abs(first[:28] - exact[:28]) / ((n + 4) * 2.0 ** -53 * mag[:28])
            print("pass 0 alone: smallest error / bound", float(miss.min()))
            assert miss.min() > 100.0


def test_recorded_recovery_and_the_qualitative_bar():
    """There is a motion for which three levels end below 1 % of the applied motion while one level at the fine gate ends above
    the applied motion.  The restatement's normals are depth_prep's, not the prototype's finite differences, and its scene is its
    own: the boundary lies elsewhere than in the prototype's table.  The motion is chosen from the JSON: size 1 (4.5 degrees and
    111 mm).  At 9 degrees and 222 mm (size 2) this scene's three levels do NOT recover; the JSON records that too."""
    with open(GOLDEN) as f:
        rec = json.load(f)
    assert tuple(rec["gates"]) == TC.GATES and tuple(rec["cosines"]) == TC.COSINES and tuple(rec["iters"]) == TC.ITERS
    r = rec["sizes"][BAR_SIZE]
    assert r["pyramid"]["deg"] < 0.01 * r["applied_deg"] and r["pyramid"]["m"] < 0.01 * r["applied_m"]
    assert r["fine"]["deg"] > r["applied_deg"] and r["fine"]["m"] > r["applied_m"]
    small = rec["sizes"]["0.5"]
    for mode in ("fine", "loose", "pyramid"):
        assert small[mode]["deg"] < 0.01 * small["applied_deg"] and small[mode]["m"] < 0.01 * small["applied_m"]
    # the figures are the restatement's: re-derived here for the bar's motion
    lw_true = TC.motion(float(BAR_SIZE))
    live, _ = TC.render(lw_true)
    for mode, args in (("pyramid", (3, TC.GATES, TC.COSINES, TC.ITERS)), ("fine", (1, TC.GATES[:1], TC.COSINES[:1], (sum(TC.ITERS),)))):
        T, stats = TC.track_np_pyramid(live, TC.IDENT, *args)
        deg, m = TC.pose_error(T, TC.IDENT, lw_true)
        print(mode, deg, m)
        assert abs(deg - r[mode]["deg"]) < 1e-6 and abs(m - r[mode]["m"]) < 1e-8
        assert int(stats[0][-1, 29]) == r[mode]["last_status"]
