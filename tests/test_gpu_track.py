"""GPU: K21, camera tracking (dfh_depth_halve, dfh_icp_track through kernels.depth_halve / kernels.icp_track) against the numpy
restatement (tests/track_np.py), and the Python layers (tracking.CameraTracker, FusionDM.track_frame, SlabFrame.step(track=True)).

Bars.  depth_halve (float32, one rounding per operation) and the per-pixel rows (fp64, one rounding per operation, stated order)
are compared BIT FOR BIT on every word, no excluded class.  The 29 sums are added on the matrix cores in a fixed order that the
restatement does not copy: each is held within (n + 4) 2^-53 sum |term| of math.fsum over the restatement's rows (n roundings of
the additions, one of the product, two of the weight's square root entering twice -- and the square root's own), the count
exactly, two runs to the same bits.  xi is bit for bit the restated Cholesky on the device's own sums; T after a step within
64 * 2^-53 * max(1, max |T|) (device and numpy sin / cos may differ by an ulp or two, through at most three products and four
sums per entry).  End to end the poses are held to that per-step bound times the number of iterations wherever the track
converges (measured: 7e-16 and 3e-16 against a bound of 1.35e-13).  The single fine level of the qualitative bar does not: it slides
along the wall through a nearly singular system, where the device's and numpy's orders of summation end 9e-11 apart; that pose is
held to the bar only (it must end above the applied motion), and the figure is printed.

Past the first pass.  icp_rows_kernel runs 256 workgroups per view; the maps of tests/track_cases.PASS_SHAPES have 255, 256, 257, 513,
289 and 561 tiles, so that a workgroup walks a second and a third tile with its accumulator alive (measured: worst error 2.4e-4
of the bound at up to 110 422 rows per view); sixteen views with sixteen T; min_count at equality and one above; the exponential
on either side of its series threshold."""
import json
import math
import os

import numpy as np
import pytest
import torch

from dynamicfusion_body_amd import kernels, scene, tracking
from dynamicfusion_body_amd.fusion_dm import FusionDM
from dynamicfusion_body_amd.pipeline import SlabFrame

import track_cases as TC
import track_np as TN

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
NAN, INF = np.nan, np.inf
SIZES = [(2, 2), (3, 5), (8, 8), (9, 65), (17, 17)]          # (17, 17): one 16 x 16 tile plus one (34 x 34 for the halving's output tile)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64)


def assert_same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = int((bits(got) != bits(want)).sum())
    assert bad == 0, "%s: %d of %d words differ" % (what, bad, want.size)


def special_depth(rng, H, W, dtype=np.float32):
    """A smooth negative map with steps, and every class of 'no measurement' sprinkled over it."""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    D = -(1.0 + 0.3 * np.sin(0.7 * x + 0.2) * np.cos(0.5 * y) + 0.5 * ((x // 3 + y // 2) % 2))
    D = D + 1e-3 * rng.standard_normal((H, W))
    D = D.astype(dtype)
    pick = rng.random((H, W))
    for lo, v in ((0.00, NAN), (0.04, INF), (0.08, -INF), (0.12, -0.0), (0.16, 0.0), (0.20, 2.5)):
        D[(pick >= lo) & (pick < lo + 0.04)] = v
    return D


# ---- dfh_depth_halve ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("size", [(2, 2), (3, 5), (8, 8), (9, 65), (34, 34), (35, 67)])
def test_depth_halve_bit_for_bit(size, dtype):
    rng = np.random.default_rng(size[0] * 100 + size[1])
    maps = [special_depth(rng, *size, dtype=dtype) for _ in range(2)]
    maps[1][0, 0] = NAN                                                   # an invalid anchor, whatever the draw
    if size[0] >= 8:
        maps[0][2:4, 2:4] = [[INF, 0.0], [NAN, 3.0]]                      # all taps invalid
        maps[0][4:6, 4:6] = [[-1.0, -1.25], [-0.75, -1.2500001]]          # a jump exactly max_jump (float32: -1.2500001 is beyond it)
        maps[1][4:6, 2:4] = [[-1.0, NAN], [-9.0, -1.125]]
    got = kernels.depth_halve([dev(m) for m in maps], 0.25).cpu().numpy()
    assert got.shape == (2, size[0] // 2, size[1] // 2)
    for v in range(2):
        assert_same_bits(got[v], TN.depth_halve(maps[v], 0.25), "view %d" % v)
    if size[0] >= 8:
        assert got[0, 1, 1] == 0.0 and got[0, 2, 2] == np.float32(-3.0) / np.float32(3.0) and got[1, 2, 1] == np.float32(-2.125) / np.float32(2.0)
    assert got[1, 0, 0] == 0.0


def test_depth_halve_sixteen_views_and_refusals():
    rng = np.random.default_rng(3)
    maps = [special_depth(rng, 6, 10) for _ in range(16)]
    got = kernels.depth_halve([dev(m) for m in maps], 0.1).cpu().numpy()
    for v in range(16):
        assert_same_bits(got[v], TN.depth_halve(maps[v], 0.1), "view %d" % v)
    with pytest.raises(ValueError):
        kernels.depth_halve([dev(m) for m in maps] + [dev(maps[0])], 0.1)
    with pytest.raises(ValueError):
        kernels.depth_halve([], 0.1)


# ---- dfh_icp_track: the rows ---------------------------------------------------------------------------------------------------

def run_icp(Dl, Nl, Dm, Nm, K, Ts, n_iters, want_rows=True, **kw):
    """Dl, Dm: (V, H, W); Nl (or None), Nm: (V, H, W, 3); Ts: (V, 3, 4).  Returns (T', stats, rows) as numpy."""
    T = dev(np.asarray(Ts, np.float64))
    stats, rows = kernels.icp_track(dev(Dl), None if Nl is None else dev(Nl), dev(Dm), dev(Nm), K, np.linalg.inv(K), T, n_iters,
                                    want_rows=want_rows, **kw)
    torch.cuda.synchronize()
    return T.cpu().numpy(), stats.cpu().numpy(), None if rows is None else rows.cpu().numpy()


def np_rows(Dl, Nl, Dm, Nm, K, Ts, max_dist=0.0, min_cos=0.0, huber=0.0):
    return np.stack([TN.icp_rows(Dl[v], None if Nl is None else Nl[v], Dm[v], Nm[v], K, np.linalg.inv(K), Ts[v], max_dist, min_cos, huber)
                     for v in range(len(Dl))])


def special_normals(rng, H, W):
    n = rng.standard_normal((H, W, 3))
    n[..., 2] = -np.abs(n[..., 2]) - 1.0
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    n[rng.random((H, W)) < 0.1] = 0.0                                     # pixels without a normal
    return n


@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("size", SIZES)
def test_rows_bit_for_bit_on_special_maps(size, gated):
    """Two views with different T; NaN, +-inf, -0.0, 0 and positive depths and zero normals on both sides."""
    H, W = size
    rng = np.random.default_rng(H * 1000 + W)
    K = np.array([[0.9 * W, 0.01, (W - 1) / 2.0], [0.0, 0.8 * W, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    Dl = np.stack([special_depth(rng, H, W) for _ in range(2)])
    Dm = np.stack([special_depth(rng, H, W) for _ in range(2)])
    Nl = np.stack([special_normals(rng, H, W) for _ in range(2)])
    Nm = np.stack([special_normals(rng, H, W) for _ in range(2)])
    Ts = np.stack([TN.apply_twist(np.array([0.02, -0.03, 0.05, 0.03, -0.02, 0.04]), TC.IDENT),
                   TN.apply_twist(np.array([-0.1, 0.05, -0.2, -0.1, 0.08, -0.05]), TC.IDENT)])
    kw = dict(max_dist=0.6, min_cos=0.3, huber=0.05) if gated else {}
    _, stats, rows = run_icp(Dl, Nl if gated else None, Dm, Nm, K, Ts, 1, **kw)
    want = np_rows(Dl, Nl if gated else None, Dm, Nm, K, Ts, **kw)
    assert_same_bits(rows, want, "rows")
    for v in range(2):
        assert stats[v, 0, 28] == (want[v][..., 7] > 0).sum()


def exact_case():
    """Maps on which the edge classes are hit EXACTLY: f = 32, cx = 8, cy = 4 (Kinv exact), the model a plane at depth 1 with
    normal (0, 0, -1), live depths 1, 1.25 and 1.5, four views whose T shifts by 0, half a pixel, one pixel right and one left."""
    H, W = 9, 17
    K = np.array([[32.0, 0.0, 8.0], [0.0, 32.0, 4.0], [0.0, 0.0, 1.0]])
    Dl = np.full((4, H, W), -1.0, np.float32)
    Dl[:, 4, :] = -1.25
    Dl[:, 6, :] = -1.5
    Dm = np.full((4, H, W), -1.0, np.float32)
    Nm = np.zeros((4, H, W, 3), np.float32)
    Nm[..., 2] = -1.0
    Nl = np.zeros((4, H, W, 3), np.float32)
    Nl[..., 2] = -2.0                                                     # not unit: c = 2, mm = 4, nn = 1
    Ts = np.stack([TC.IDENT.copy() for _ in range(4)])
    Ts[1, 0, 3], Ts[2, 0, 3], Ts[3, 0, 3] = 0.5 / 32, 1.0 / 32, -1.0 / 32
    return K, Dl, Nl, Dm, Nm, Ts


def test_rows_bit_for_bit_on_exact_edges():
    """u exactly on x.5 in both parities, ui exactly 0 and W - 1 (and one beyond either), d2 exactly at the gate, the cosine test
    exactly at equality, |r| exactly huber -- each checked to EXIST in the restatement, then all words compared."""
    K, Dl, Nl, Dm, Nm, Ts = exact_case()
    kw = dict(max_dist=0.25, min_cos=1.0, huber=0.25)
    want = np_rows(Dl, Nl, Dm, Nm, K, Ts, **kw)
    w = want[..., 7]
    # view 0: depth-1 rows have r == 0; on row 4 (depth 1.25) only the principal column has d2 == 0.0625 == max_dist^2 and passes
    assert np.all(w[0, 0] == 1.0) and np.all(want[0, 0, :, 6] == 0.0)
    assert w[0, 4, 8] == 1.0 and want[0, 4, 8, 6] == -0.25 and not w[0, 4, :8].any() and not w[0, 4, 9:].any()
    assert not w[0, 6].any()                                              # depth 1.5: beyond the gate
    # view 1: u = x + 0.5 exactly; half to even sends even x to x and odd x to x + 1: the last column (x = 16) stays inside
    assert np.all(w[1, 0] == 1.0)
    # views 2, 3: one pixel right / left: the far column leaves the image, ui == W - 1 and ui == 0 are hit
    assert not w[2, 0, 16] and w[2, 0, 15] and not w[3, 0, 0] and w[3, 0, 1]
    _, stats, rows = run_icp(Dl, Nl, Dm, Nm, K, Ts, 1, **kw)
    assert_same_bits(rows, want, "rows")
    # without the distance gate the Huber classes show: |r| == huber exactly keeps w = 1, |r| = 0.5 gets w = 0.5
    kw = dict(max_dist=0.0, min_cos=1.0, huber=0.25)
    want = np_rows(Dl, Nl, Dm, Nm, K, Ts, **kw)
    assert np.all(want[0, 4, :, 6] == -0.25) and np.all(want[0, 4, :, 7] == 1.0)
    assert np.all(want[0, 6, :, 6] == -0.5) and np.all(want[0, 6, :, 7] == 0.5)
    assert_same_bits(run_icp(Dl, Nl, Dm, Nm, K, Ts, 1, **kw)[2], want, "rows, huber")
    # the cosine exactly at equality passes; one ulp more of min_cos is past float64's 1.0: a live normal tilted by a hair fails
    Nl2 = Nl.copy()
    Nl2[:, 0, :, 0] = 2.0 ** -10
    want = np_rows(Dl, Nl2, Dm, Nm, K, Ts, **kw)
    assert not want[0, 0, :, 7].any() and want[0, 1, :, 7].all()
    assert_same_bits(run_icp(Dl, Nl2, Dm, Nm, K, Ts, 1, **kw)[2], want, "rows, cosine")


def test_rows_behind_the_camera_and_identical_maps():
    md, mn = TC.render(TC.IDENT)
    Dl, Nm = np.stack([md, md]), np.stack([mn, mn])
    behind = TC.IDENT.copy()
    behind[2, 3] = -5.0                                                   # every live point behind the model camera: q_2 < 0
    Ts = np.stack([TC.IDENT, behind])
    want = np_rows(Dl, Nm, Dl, Nm, TC.K, Ts, max_dist=0.1, min_cos=0.8)
    assert (want[0][..., 7] > 0).sum() > 15000 and not want[0][..., 6].any()       # identical maps under the identity: r == 0
    assert not want[1].any()
    T1, stats, rows = run_icp(Dl, Nm, Dl, Nm, TC.K, Ts, 2, max_dist=0.1, min_cos=0.8, lm_rel=1e-3)
    assert_same_bits(rows, want, "rows")
    assert stats[0, 0, 29] == 1.0 and not stats[0, 0, 21:28].any() and not stats[0, 0, 30:36].any()   # g == 0: a step of zero
    assert_same_bits(T1[0], TC.IDENT, "T under a zero step")
    assert not stats[1].any() and np.array_equal(T1[1], behind)                                        # no rows: refused


# ---- the sums, the solve, the refusals ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene_frame():
    """Model = the scene from the identity, live = the scene from motion(0.3) with the restatement's normals; two views, the
    second with a prior that is already half way."""
    lw = TC.motion(0.3)
    live, _ = TC.render(lw)
    (_, D, n), = TC.live_pyramid(live, 1)
    md, mn = TC.render(TC.IDENT)
    Ts = np.stack([TC.IDENT, TN.invert_rigid(TC.motion(0.15))])
    return np.stack([D, D]), np.stack([n, n]), np.stack([md, md]), np.stack([mn, mn]), Ts


def test_sums_within_the_rounding_bound_and_repeatable(scene_frame):
    Dl, Nl, Dm, Nm, Ts = scene_frame
    kw = dict(max_dist=0.1, min_cos=0.8, huber=0.01, lm_rel=1e-3)
    T1, stats, rows = run_icp(Dl, Nl, Dm, Nm, TC.K, Ts, 1, **kw)
    want = np_rows(Dl, Nl, Dm, Nm, TC.K, Ts, max_dist=0.1, min_cos=0.8, huber=0.01)
    assert_same_bits(rows, want, "rows")
    for v in range(2):
        exact, mag = TN.icp_sums(want[v])
        n = int(exact[28])
        assert n > 5000 and (want[v][..., 7] < 1.0).sum() > 100                     # Huber weights take part
        assert stats[v, 0, 28] == n
        err = np.abs(stats[v, 0, :28] - exact[:28])
        bound = (n + 4) * EPS * mag[:28]
        print("view", v, "rows", n, "worst error / bound", float((err / bound).max()))
        assert np.all(err <= bound)
    T2, stats2, _ = run_icp(Dl, Nl, Dm, Nm, TC.K, Ts, 1, **kw)
    assert_same_bits(stats2, stats, "stats of a second run")
    assert_same_bits(T2, T1, "T of a second run")


def test_solve_bit_for_bit_on_the_device_sums(scene_frame):
    Dl, Nl, Dm, Nm, Ts = scene_frame
    kw = dict(max_dist=0.1, min_cos=0.8, huber=0.01, lm_rel=1e-3, min_count=100, max_rot=0.5, max_trans=0.5)
    T1, stats, _ = run_icp(Dl, Nl, Dm, Nm, TC.K, Ts, 1, want_rows=False, **kw)
    for v in range(2):
        status, xi, Tn = TN.icp_solve(stats[v, 0, :29], Ts[v], 1e-3, 100, 0.5, 0.5)
        assert status == 1 and stats[v, 0, 29] == 1.0 and not stats[v, 0, 36:].any()
        assert_same_bits(stats[v, 0, 30:36], xi, "xi")
        err = float(np.abs(T1[v] - Tn).max())
        bound = 64 * EPS * max(1.0, float(np.abs(Tn).max()))
        print("view", v, "T error", err, "bound", bound)
        assert err <= bound
    # chained: the second iteration reads the first one's T
    T2, stats2, _ = run_icp(Dl, Nl, Dm, Nm, TC.K, Ts, 2, want_rows=False, **kw)
    assert_same_bits(stats2[:, 0], stats[:, 0], "first record of two")
    assert_same_bits(run_icp(Dl, Nl, Dm, Nm, TC.K, T1, 1, want_rows=False, **kw)[1][:, 0], stats2[:, 1], "second record")


def test_refusals_leave_T_untouched(scene_frame):
    Dl, Nl, Dm, Nm, Ts = scene_frame
    base = dict(max_dist=0.1, min_cos=0.8, lm_rel=1e-3)
    for kw in (dict(min_count=10 ** 6), dict(max_rot=1e-9), dict(max_trans=1e-9)):
        T1, stats, _ = run_icp(Dl, Nl, Dm, Nm, TC.K, Ts, 3, want_rows=False, **dict(base, **kw))
        assert_same_bits(T1, Ts, "T after %r" % (kw,))
        assert stats[:, :, 28].min() > 5000 and not stats[:, :, 29:].any()
        assert_same_bits(stats[:, 1], stats[:, 0], "the refusal repeats")
        assert_same_bits(stats[:, 2], stats[:, 0], "and again")
    # a singular system: one plane facing the camera, no damping -- the in-plane translations have A_33 = A_44 = 0 exactly
    z = np.full((1, 24, 32), -1.5, np.float32)
    nz = np.zeros((1, 24, 32, 3), np.float32)
    nz[..., 2] = -1.0
    Kp = np.array([[30.0, 0, 15.5], [0, 30.0, 11.5], [0, 0, 1]])
    T0 = TC.IDENT[None].copy()
    T0[0, 2, 3] = 0.01
    T1, stats, _ = run_icp(z, nz, z, nz, Kp, T0, 2, want_rows=False, lm_rel=0.0)
    assert stats[0, 0, 28] == 24 * 32 and stats[0, 0, 27] > 0 and not stats[0, :, 29:].any()
    assert TN.icp_solve(stats[0, 0, :29], T0[0], 0.0, 6, math.inf, math.inf)[0] == 0
    assert_same_bits(T1, T0, "T of the singular system")


# ---- past the first pass of the rows grid: a workgroup walks a second and a third tile -----------------------------------------

def assert_sums_within_bound(rec, want_rows, what):
    """One (view, iteration) record against the restatement's rows: the count exactly, the 28 sums within (n + 4) 2^-53 sum |term|."""
    exact, mag = TN.icp_sums(want_rows)
    n = int(exact[28])
    assert rec[28] == n, "%s: count %r, restated %d" % (what, rec[28], n)
    err = np.abs(rec[:28] - exact[:28])
    bound = (n + 4) * EPS * mag[:28]
    print(what, "rows", n, "worst error / bound", float((err / bound).max()) if n else 0.0)
    assert np.all(err <= bound), what
    return n


@pytest.mark.parametrize("size", list(TC.PASS_SHAPES))
def test_rows_and_sums_past_the_first_pass(size):
    """255, 256, 257, 513, 289 and 561 tiles against the grid's 256 workgroups per view: zero or one tile each, exactly one, one
    workgroup two, one three, a two-dimensional map, and a partial third pass that ends in a one-pixel-high tile row.  The MFMA
    accumulator lives across the passes and the LDS rows are rewritten for every tile behind a wave barrier only: rows bit for bit,
    the count exactly, the sums within the bound, a second run to the same bits, xi bit for bit on the device's sums.
    tests/test_track_np.py::test_pass_cases_reach_every_pass_of_the_rows_grid holds the maps to their purpose (a row in every
    pass, pass 0 alone outside this bound)."""
    H, W = size
    tiles, passes = TC.PASS_SHAPES[size]
    assert TC.n_tiles(H, W) == tiles and -(-tiles // TC.ICP_GRID) == passes
    c = TC.pass_case(H, W)
    kw = dict(TC.PASS_GATES, lm_rel=1e-3)
    args = (c["Dl"], c["Nl"], c["Dm"], c["Nm"], c["K"], c["Ts"])
    T1, stats, rows = run_icp(*args, 1, **kw)
    assert_same_bits(rows, c["rows"], "rows")
    for v in range(2):
        assert assert_sums_within_bound(stats[v, 0], c["rows"][v], "%r view %d" % (size, v)) > 0.5 * H * W
        status, xi, Tn = TN.icp_solve(stats[v, 0, :29], c["Ts"][v], 1e-3, 6, math.inf, math.inf)
        assert status == 1 and stats[v, 0, 29] == 1.0 and not stats[v, 0, 36:].any()
        assert_same_bits(stats[v, 0, 30:36], xi, "xi")
        assert float(np.abs(T1[v] - Tn).max()) <= 64 * EPS * max(1.0, float(np.abs(Tn).max()))
    T2, stats2, rows2 = run_icp(*args, 1, **kw)
    assert_same_bits(stats2, stats, "stats of a second run")
    assert_same_bits(T2, T1, "T of a second run")
    assert_same_bits(rows2, rows, "rows of a second run")


def test_chained_iterations_past_the_first_pass():
    """Three iterations in one call on the 289-tile map, no rows written: record i is the first record of a fresh one-iteration
    call started from the T the records before it left (the partial sets and the accumulators carry nothing from one iteration
    to the next), and each record's sums are within the bound of the restatement's rows at that T."""
    c = TC.pass_case(272, 272)
    kw = dict(TC.PASS_GATES, lm_rel=1e-3, min_count=100, max_rot=0.5, max_trans=0.5)
    args = (c["Dl"], c["Nl"], c["Dm"], c["Nm"], c["K"])
    T3, stats3, none = run_icp(*args, c["Ts"], 3, want_rows=False, **kw)
    assert none is None and np.all(stats3[:, :, 29] == 1.0)
    T = c["Ts"]
    for i in range(3):
        want = np_rows(*args, T, **TC.PASS_GATES)
        for v in range(2):
            assert_sums_within_bound(stats3[v, i], want[v], "iteration %d view %d" % (i, v))
        T, stats, _ = run_icp(*args, T, 1, want_rows=False, **kw)
        assert_same_bits(stats[:, 0], stats3[:, i], "record %d" % i)
    assert_same_bits(T, T3, "T after three iterations")
    assert not np.array_equal(stats3[:, 0, :28], stats3[:, 1, :28]) and not np.array_equal(stats3[:, 1, :28], stats3[:, 2, :28])


# ---- sixteen views ---------------------------------------------------------------------------------------------------------------

def test_sixteen_views_each_with_its_own_maps_and_T():
    """The view index scales the maps' base, T, the partial sets and the records: sixteen views of 34 x 50 (3 x 4 tiles, the last
    row and column of tiles two pixels wide), every map drawn on its own, sixteen different T, one view without a live measurement.
    Rows bit for bit, counts exactly, sums within the bound per view, xi bit for bit on each view's own sums; seventeen views are
    refused by icp_track and by icp_track_scratch."""
    V, H, W, BLANK = 16, 34, 50, 11
    K = np.array([[0.9 * W, 0.01, (W - 1) / 2.0], [0.0, 0.8 * W, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    Dl, Nl, Dm, Nm, Ts = [], [], [], [], []
    for v in range(V):
        rng = np.random.default_rng(7000 + v)
        Dl.append(special_depth(rng, H, W)); Dm.append(special_depth(rng, H, W))
        Nl.append(special_normals(rng, H, W)); Nm.append(special_normals(rng, H, W))
        Ts.append(TN.apply_twist(rng.normal(scale=[0.03] * 3 + [0.05] * 3), TC.IDENT))
    Dl, Nl, Dm, Nm, Ts = (np.stack(a) for a in (Dl, Nl, Dm, Nm, Ts))
    Dl[BLANK] = 0.0
    assert len({T.tobytes() for T in Ts}) == V
    kw = dict(max_dist=0.6, min_cos=0.3, huber=0.05)
    want = np_rows(Dl, Nl, Dm, Nm, K, Ts, **kw)
    T1, stats, rows = run_icp(Dl, Nl, Dm, Nm, K, Ts, 1, lm_rel=1e-3, **kw)
    assert_same_bits(rows, want, "rows")
    counts = []
    for v in range(V):
        counts.append(assert_sums_within_bound(stats[v, 0], want[v], "view %d" % v))
        status, xi, Tn = TN.icp_solve(stats[v, 0, :29], Ts[v], 1e-3, 6, math.inf, math.inf)
        assert stats[v, 0, 29] == status
        assert_same_bits(stats[v, 0, 30:36], xi, "xi of view %d" % v)
        assert float(np.abs(T1[v] - Tn).max()) <= 64 * EPS * max(1.0, float(np.abs(Tn).max()))
    assert counts[BLANK] == 0 and not stats[BLANK].any()
    assert_same_bits(T1[BLANK], Ts[BLANK], "T of the view without a live map")
    stepped = [v for v in range(V) if stats[v, 0, 29] == 1.0]
    assert len(stepped) >= 12 and len(set(counts)) >= 12                  # (the views do differ: a view reading another's maps shows)
    for v in stepped:
        assert not np.array_equal(T1[v], Ts[v])
    with pytest.raises(ValueError):
        kernels.icp_track_scratch(V + 1)
    more = [np.concatenate([a, a[:1]]) for a in (Dl, Nl, Dm, Nm, Ts)]
    with pytest.raises(ValueError):                                      # (its own scratch: icp_track_scratch refuses first)
        run_icp(*more[:4], K, more[4], 1, **kw)
    T17 = dev(more[4])
    with pytest.raises(ValueError, match="views"):                       # (a scratch that exists: the library refuses)
        kernels.icp_track(dev(more[0]), dev(more[1]), dev(more[2]), dev(more[3]), K, np.linalg.inv(K), T17, 1,
                          scratch=kernels.icp_track_scratch(V), **kw)
    assert_same_bits(T17.cpu().numpy(), more[4], "T of a refused call")


# ---- the finish kernel's two decisions at their edges -------------------------------------------------------------------------

def test_min_count_at_its_edge(scene_frame):
    """sv[28] >= min_count decides per view: with min_count equal to a view's count that view steps (the record is the unconstrained
    run's, bit for bit), with one more it is refused (T untouched, the record zero from index 29 on).  The two views' counts
    differ, so one call holds a view that steps beside one that is refused."""
    Dl, Nl, Dm, Nm, Ts = scene_frame
    base = dict(max_dist=0.1, min_cos=0.8, huber=0.01, lm_rel=1e-3)
    T_free, free, _ = run_icp(Dl, Nl, Dm, Nm, TC.K, Ts, 1, want_rows=False, **base)
    n = [int(free[v, 0, 28]) for v in range(2)]
    assert n[0] != n[1] and min(n) > 5000 and np.all(free[:, 0, 29] == 1.0)
    lo, hi = (0, 1) if n[0] < n[1] else (1, 0)
    for min_count, steps in ((n[lo], (lo, hi)), (n[lo] + 1, (hi,)), (n[hi], (hi,)), (n[hi] + 1, ())):
        T1, stats, _ = run_icp(Dl, Nl, Dm, Nm, TC.K, Ts, 1, want_rows=False, min_count=min_count, **base)
        assert_same_bits(stats[:, 0, :29], free[:, 0, :29], "sums at min_count %d" % min_count)
        for v in range(2):
            if v in steps:
                assert stats[v, 0, 29] == 1.0
                assert_same_bits(stats[v, 0], free[v, 0], "record of the stepping view %d at min_count %d" % (v, min_count))
                assert_same_bits(T1[v], T_free[v], "T of the stepping view")
            else:
                assert not stats[v, 0, 29:].any(), (v, min_count)
                assert_same_bits(T1[v], Ts[v], "T of the refused view")
            assert TN.icp_solve(stats[v, 0, :29], Ts[v], 1e-3, min_count, math.inf, math.inf)[0] == (1 if v in steps else 0)


def test_small_angle_branch_of_the_exponential():
    """The model as the live map under a prior that is a pure rotation: of 5e-5 rad in view 0, whose step lands below the series
    branch's ww < 1e-8, and of 2e-4 rad in view 1, above it (ww read from the device's xi).  xi bit for bit on the device's sums,
    T within 64 * 2^-53 * max(1, max |T|) of the restated exponential on either branch, and bit for bit through the series branch.
    (At ww = 4e-8 the two branches' a, b, c agree to ww^2 / 120 = 1e-17, below an ulp: moving the threshold there changes T by
    rounding only, which the bound allows -- a threshold of 1e-7 is not told from 1e-8 by any bound on T.)"""
    md, mn = TC.render(TC.IDENT)
    axis = np.array([0.3, 1.0, 0.2]) / np.linalg.norm([0.3, 1.0, 0.2])
    Ts = np.stack([TN.apply_twist(np.concatenate([a * axis, np.zeros(3)]), TC.IDENT) for a in (5e-5, 2e-4)])
    D, N = np.stack([md, md]), np.stack([mn, mn])
    kw = dict(max_dist=0.1, min_cos=0.8, huber=0.01, lm_rel=1e-3, min_count=100, max_rot=0.5, max_trans=0.5)
    T1, stats, _ = run_icp(D, N, D, N, TC.K, Ts, 1, want_rows=False, **kw)
    ww = [float((stats[v, 0, 30] * stats[v, 0, 30] + stats[v, 0, 31] * stats[v, 0, 31]) + stats[v, 0, 32] * stats[v, 0, 32]) for v in range(2)]
    print("ww", ww)
    assert 0.0 < ww[0] < 1e-8 < ww[1]
    for v in range(2):
        status, xi, Tn = TN.icp_solve(stats[v, 0, :29], Ts[v], 1e-3, 100, 0.5, 0.5)
        assert status == 1 and stats[v, 0, 29] == 1.0 and stats[v, 0, 28] > 15000
        assert_same_bits(stats[v, 0, 30:36], xi, "xi")
        err = float(np.abs(T1[v] - Tn).max())
        bound = 64 * EPS * max(1.0, float(np.abs(Tn).max()))
        print("view", v, "T error", err, "bound", bound, "same bits", bool(np.array_equal(T1[v], Tn)))
        assert err <= bound and not np.array_equal(T1[v], Ts[v])
    # the series branch calls neither sin nor cos: every operation of it rounds once, in the stated order
    assert_same_bits(T1[0], TN.icp_solve(stats[0, 0, :29], Ts[0], 1e-3, 100, 0.5, 0.5)[2], "T through the series branch")


def test_no_iterations_launch_nothing(scene_frame):
    Dl, Nl, Dm, Nm, Ts = scene_frame
    T1, stats, rows = run_icp(Dl, Nl, Dm, Nm, TC.K, Ts, 0)
    assert stats.shape == (2, 0, 40) and rows is None
    assert_same_bits(T1, Ts, "T")


# ---- the Python layers -------------------------------------------------------------------------------------------------------

def analytic_model(lws, K, H, W):
    maps = [TC.render(lw, K, H, W) for lw in lws]
    return dev(np.stack([m[0] for m in maps])), dev(np.stack([m[1] for m in maps]))


def step_bound(T, iters):
    return iters * 64 * EPS * max(1.0, float(np.abs(T).max()))


def test_camera_tracker_against_the_restatement_and_the_bar():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_recovery.json")) as f:
        rec = json.load(f)["sizes"]["1"]
    lw_true = TC.motion(1.0)
    live, _ = TC.render(lw_true)
    total = sum(TC.ITERS)
    pyramid = tracking.CameraTracker(TC.K, 3, TC.ITERS, TC.GATES, TC.COSINES, max_jump=TC.MAX_JUMP, lm_rel=TC.LM_REL)
    fine = tracking.CameraTracker(TC.K, 1, (total,), TC.GATES[:1], TC.COSINES[:1], max_jump=TC.MAX_JUMP, lm_rel=TC.LM_REL)
    # the live pyramid is the restatement's, bit for bit
    for (d, n), (_, dn, nn) in zip(pyramid.live_pyramid([live]), TC.live_pyramid(live, 3)):
        assert_same_bits(d[0].cpu().numpy(), dn, "pyramid depth")
        assert_same_bits(n[0].cpu().numpy(), nn, "pyramid normals")
    out = {}
    for name, tr, args in (("pyramid", pyramid, (3, TC.GATES, TC.COSINES, TC.ITERS)), ("fine", fine, (1, TC.GATES[:1], TC.COSINES[:1], (total,)))):
        lws, stats = tr.track([live], [TC.IDENT], analytic_model)
        Tn, sn = TC.track_np_pyramid(live, TC.IDENT, *args)
        err = float(np.abs(stats["T"][0] - Tn).max())
        print(name, "T error", err, "bound", step_bound(Tn, total), "statuses", [s[0][:, 29].tolist() for s in stats["levels"]])
        for l in range(len(sn)):
            assert np.array_equal(stats["levels"][l][0][:, 28:30], sn[l][:, 28:30])              # counts and statuses
        assert not stats["lost"][0]
        if name == "pyramid":        # (the single fine level slides along the wall: a pose that is no fixed point has no such bound)
            assert err <= step_bound(Tn, total)
            want = TN.compose(TN.invert_rigid(np.concatenate([TN.project_so3(Tn[:, :3]), Tn[:, 3:]], axis=1)), TC.IDENT)
            assert float(np.abs(lws[0] - want).max()) <= 4 * step_bound(Tn, total)
        out[name] = TC.pose_error(np.concatenate([tracking.project_so3(stats["T"][0][:, :3]), stats["T"][0][:, 3:]], axis=1), TC.IDENT, lw_true)
    print(out)
    assert out["pyramid"][0] < 0.01 * rec["applied_deg"] and out["pyramid"][1] < 0.01 * rec["applied_m"]
    assert out["fine"][0] > rec["applied_deg"] and out["fine"][1] > rec["applied_m"]


def test_camera_tracker_marks_a_lost_view():
    live, _ = TC.render(TC.motion(0.3))
    blank = np.zeros_like(live)
    tr = tracking.CameraTracker(TC.K, 2, (2, 2), TC.GATES[:2], TC.COSINES[:2], max_jump=TC.MAX_JUMP, lm_rel=TC.LM_REL)
    prior = [TC.IDENT, TC.motion(0.1)]
    lws, stats = tr.track([live, blank], prior, analytic_model)
    assert stats["lost"].tolist() == [False, True]
    assert np.array_equal(lws[1], prior[1]) and not np.array_equal(lws[0], prior[0])


R64 = 64


def test_fusion_dm_track_frame():
    """A 64^3 volume fused from pose A; a frame from pose B, prior A, is tracked to the pose the restatement finds on the device's
    own ray-cast maps."""
    scale, center = 1.6 / R64, np.array([0.0, 0.0, 1.4])
    tdist = 4.0 * scale
    lw_a, lw_b = TC.IDENT, TC.motion(0.3)
    Kinv = np.linalg.inv(TC.K)
    T = torch.full((R64, R64, R64), tdist / scale, dtype=torch.float32, device="cuda")
    Wt = torch.zeros_like(T)
    kernels.integrate_depth(T, Wt, dev(TC.render(lw_a)[0]), TC.K, Kinv, lw_a, scale, center, tdist)
    fdm = FusionDM(tdist, TC.K, tsdf_res=R64)
    fdm._T, fdm._Wt = T, Wt
    live = TC.render(lw_b)[0]
    tr = tracking.CameraTracker(TC.K, 3, TC.ITERS, TC.GATES, TC.COSINES, max_jump=TC.MAX_JUMP, lm_rel=TC.LM_REL)
    lws, stats = fdm.track_frame([live], [lw_a], tr, scale=scale, center=center, min_weight=1.0)

    def device_model(lw_prev, K, H, W):
        r = fdm.render_model([lw_prev], H, W, K=K, scale=scale, center=center, min_weight=1.0, want=("depth", "normals"))
        return r.depth[0].cpu().numpy(), r.normals[0].cpu().numpy()
    Tn, sn = TC.track_np_pyramid(live, lw_a, 3, TC.GATES, TC.COSINES, TC.ITERS, model=device_model)
    total = sum(TC.ITERS)
    err = float(np.abs(stats["T"][0] - Tn).max())
    before, after = TC.pose_error(TC.IDENT, lw_a, lw_b), TC.pose_error(stats["T"][0], lw_a, lw_b)
    print("T error", err, "bound", step_bound(Tn, total), "pose error before", before, "after", after)
    assert sn[0][-1, 28] > 3000 and not stats["lost"][0]
    assert err <= step_bound(Tn, total)
    want = TN.compose(TN.invert_rigid(np.concatenate([TN.project_so3(Tn[:, :3]), Tn[:, 3:]], axis=1)), lw_a)
    assert float(np.abs(lws[0] - want).max()) <= 4 * step_bound(Tn, total)
    # (a model on a 25 mm voxel grid seen from one side: a few millimetres remain of the 33 mm applied, not the analytic model's figure)
    assert after[0] < 0.5 * before[0] and after[1] < 0.5 * before[1]


def _loop(K, lws, first, R=32, **kw):
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(24, R)
    sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=4, band=2.0, distributed=False, **kw)
    for d, lw in zip(first, lws):
        sf.integrate(d, lw)
    assert sf.refresh_samples() > 100
    return sf


@pytest.mark.parametrize("model", ["live", "mesh"])
def test_slab_frame_tracks_its_cameras(model, monkeypatch):
    """step(track=True) with a perturbed prior = the tracker's calls, then the very frame a loop without a tracker runs when it
    is GIVEN the tracked cameras: volumes and warp field agree bit for bit.  With track unset the tracker is never reached."""
    H, W = 60, 80
    K = scene.intrinsics(75.0, 39.5, 29.5)
    lws = [scene.view_extrinsic(0.0), scene.view_extrinsic(40.0)]
    frames = [[torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0,
                                                   sphere_offset=np.array([0.01 * f, 0.0, 0.0]))).cuda() for lw in lws] for f in range(3)]
    scale = scene.grid_params(32)[0]
    tr = tracking.CameraTracker(K, 2, (3, 3), (4 * scale, 8 * scale), (0.7, 0.5), max_jump=2 * scale, min_count=50)
    calls = {"icp": 0, "halve": 0}
    real_icp, real_halve = kernels.icp_track, kernels.depth_halve
    monkeypatch.setattr(kernels, "icp_track", lambda *a, **k: calls.__setitem__("icp", calls["icp"] + 1) or real_icp(*a, **k))
    monkeypatch.setattr(kernels, "depth_halve", lambda *a, **k: calls.__setitem__("halve", calls["halve"] + 1) or real_halve(*a, **k))
    a = _loop(K, lws, frames[0], tracker=tr, track_model=model)
    b = _loop(K, lws, frames[0])
    assert a.step(frames[1], lws, gn_iters=2) == b.step(frames[1], lws, gn_iters=2)
    assert calls == {"icp": 0, "halve": 0} and a.tracked_lw is None
    prior = [TN.compose(TN.apply_twist(np.array([0.004, -0.006, 0.003, 0.01, -0.005, 0.008]), TC.IDENT), lw) for lw in lws]
    na = a.step(frames[2], prior, gn_iters=2, track=True)
    assert calls == {"icp": 2, "halve": 1}                                           # one call per level, one halving
    assert len(a.tracked_lw) == 2 and a.track_stats["T"].shape == (2, 3, 4)
    print(model, "lost", a.track_stats["lost"].tolist(), "counts", a.track_stats["levels"][0][:, -1, 28].tolist())
    for v in range(2):
        moved = not np.array_equal(a.tracked_lw[v], prior[v])
        assert moved != bool(a.track_stats["lost"][v])
    assert not a.track_stats["lost"].all()
    nb = b.step(frames[2], a.tracked_lw, gn_iters=2)
    torch.cuda.synchronize()
    assert na == nb
    assert torch.equal(a.T, b.T) and torch.equal(a.Wt, b.Wt) and torch.equal(a.fs.solver.node_dq, b.fs.solver.node_dq)
    with pytest.raises(ValueError, match="tracker"):
        b.step(frames[2], lws, gn_iters=2, track=True)
