"""GPU: the volume data term -- dfh_gn_associate_volume and the layers above it (WarpSolver.associate_volume / iterate_volume,
FrameSolver.*_volume, SlabFrame.step(data_term="volume"), Fusion.setupCorrespondences / solve(method='sdf')).

`restate` below is the numpy restatement of the definition in include/dfusion_hip.h (fp64, operation by operation; numpy does
not contract a * b + c); the samples are warped with oracle_np.warp as tests/test_gpu_solve.py::test_projective_association_vs_oracle
does."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import gn_np as G
from oracle import oracle_np as O
from dynamicfusion_body_amd import kernels, scene, solve
from dynamicfusion_body_amd.pipeline import FrameSolver, SlabFrame

pytestmark = pytest.mark.gpu

IDENT = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
OUT_OF_GRID, OUT_OF_BAND, NO_GRADIENT, GATED, VALID = range(5)


def restate(xw, live, value_to_vox=1.0, band=4.0, max_dist=0.0, min_grad=0.5):
    """The definition of dfh_gn_associate_volume for warped points xw (S, 3) -> (corr, valid, outcome, margin, s).
    margin: how far the decision is from flipping under a perturbation of xw -- the distance of a coordinate to the nearest
    integer plane (a cell face or the grid's boundary), and for the samples that reach them the slack of the gradient test and of
    the gate.  s: the interpolant's value (NaN outside the grid)."""
    xw = np.asarray(xw, dtype=np.float64)
    S = xw.shape[0]
    res = live.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        in_grid = np.ones(S, dtype=bool)
        for a in range(3):
            in_grid &= np.isfinite(xw[:, a]) & (0.0 <= xw[:, a]) & (xw[:, a] < res[a] - 1)
        X = np.where(in_grid[:, None], xw, 0.0)
        fl = np.floor(X)
        i = fl.astype(np.int64)
        f0, f1, f2 = (X - fl).T
        u = np.empty((2, 2, 2, S))
        for a in range(2):
            for b in range(2):
                for c in range(2):
                    u[a, b, c] = live[i[:, 0] + a, i[:, 1] + b, i[:, 2] + c].astype(np.float64) * value_to_vox
        in_band = np.ones(S, dtype=bool)
        for a in range(2):
            for b in range(2):
                for c in range(2):
                    in_band &= np.abs(u[a, b, c]) < band
        e = u[:, :, 0] + f2 * (u[:, :, 1] - u[:, :, 0])
        h = e[:, 0] + f1 * (e[:, 1] - e[:, 0])
        s = h[0] + f0 * (h[1] - h[0])
        g0 = h[1] - h[0]
        dy = e[:, 1] - e[:, 0]
        g1 = dy[0] + f0 * (dy[1] - dy[0])
        dz = u[:, :, 1] - u[:, :, 0]
        m = dz[:, 0] + f1 * (dz[:, 1] - dz[:, 0])
        g2 = m[0] + f0 * (m[1] - m[0])
        Gq = (g0 * g0 + g1 * g1) + g2 * g2
        grad_ok = (Gq >= min_grad * min_grad) & (Gq > 0.0)
        gate_ok = (s * s <= (max_dist * max_dist) * Gq) if max_dist > 0 else np.ones(S, dtype=bool)
        valid = in_grid & in_band & grad_ok & gate_ok
        t = s / Gq
        corr = np.where(valid[:, None], xw - t[:, None] * np.stack([g0, g1, g2], axis=1), 0.0)
        outcome = np.full(S, VALID)
        outcome[~gate_ok] = GATED
        outcome[~grad_ok] = NO_GRADIENT
        outcome[~in_band] = OUT_OF_BAND
        outcome[~in_grid] = OUT_OF_GRID
        margin = np.abs(xw - np.rint(xw)).min(axis=1)
        margin = np.where(np.isfinite(margin), margin, np.inf)
        reach = in_grid & in_band
        margin = np.where(reach, np.minimum(margin, np.abs(Gq - min_grad * min_grad)), margin)
        if max_dist > 0:
            margin = np.where(reach & grad_ok, np.minimum(margin, np.abs(s * s - (max_dist * max_dist) * Gq)), margin)
    return corr, valid, outcome, margin, np.where(in_grid, s, np.nan)


def sphere_volume(R, centre, radius, trunc=4.0):
    X, Y, Z = np.meshgrid(*(np.arange(R, dtype=np.float64),) * 3, indexing="ij")
    sd = np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - radius
    return np.where(sd > -trunc, np.minimum(trunc, sd), trunc)


_SCENE = {}


def sphere_scene():
    """R = 32 sphere volume (fp64 master; the float32 volume is its rounding), 40 Fibonacci nodes with random twists, a random lw."""
    if not _SCENE:
        R = 32
        rng = np.random.default_rng(7)
        npos, nw = scene.fibonacci_nodes(40, R)
        ndq = np.array([G.twist_exp_dq(rng.normal(size=6) * np.array([.02, .02, .02, .5, .5, .5])) for _ in range(40)])
        lw = G.twist_exp_dq(np.array([0.01, -0.02, 0.015, 0.3, -0.2, 0.1]))
        centre, radius = np.array([15.3, 16.1, 15.7]), 9.5
        _SCENE.update(R=R, npos=npos, nw=nw, ndq=ndq, lw=lw, centre=centre, radius=radius, live=sphere_volume(R, centre, radius))
    return _SCENE


def ray_samples(S, sc):
    rng = np.random.default_rng(11)
    d = rng.normal(size=(S, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = sc["centre"] + d * sc["radius"] * rng.uniform(0.45, 1.6, size=(S, 1))
    pts[:200] = rng.uniform(-2.0, 33.0, size=(200, 3))
    return pts, d


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("k,S", [(4, 4000), (1, 500), (8, 500)])
def test_volume_association_vs_restatement(dtype, k, S):
    sc = sphere_scene()
    live = sc["live"].astype(dtype)
    live_t = torch.from_numpy(live).cuda()
    pts, d = ray_samples(S, sc)
    sv = solve.WarpSolver(knn=k)
    sv.set_graph(sc["npos"], sc["ndq"], sc["nw"])
    sv.set_samples(pts, d, sort=False)
    loc = sv.snbr.cpu().numpy().astype(np.int64)
    warped = O.warp(pts, sc["ndq"][loc], sc["npos"][loc], sc["nw"][loc], m_lw=sc["lw"])
    seen = set()
    for max_dist in (0.0, 2.0):
        sv.corr.fill_(7.0)                                       # every row is written: nothing of this survives
        sv.valid.fill_(3)
        sv.associate_volume(live_t, sc["lw"], band=4.0, max_dist=max_dist, min_grad=0.5)
        corr, valid = sv.corr.cpu().numpy(), sv.valid.cpu().numpy()
        co, vo, outcome, margin, _ = restate(warped, live, 1.0, 4.0, max_dist, 0.5)
        sure = margin > 1e-9
        print("dtype %s knn %d max_dist %g: outcomes %s, left out %d, smallest margin %.3g, max |corr - restated| %.3g" % (
            np.dtype(dtype).name, k, max_dist, np.bincount(outcome, minlength=5).tolist(), int((~sure).sum()), margin.min(),
            np.abs(corr - co)[sure & vo].max()))
        assert (~sure).sum() <= 0.001 * S
        assert set(np.unique(valid).tolist()) <= {0, 1}
        assert np.array_equal(valid[sure].astype(bool), vo[sure])
        both = valid.astype(bool) & vo
        assert np.abs(corr[both] - co[both]).max() <= 1e-9
        assert np.all(corr[valid == 0] == 0.0)
        seen |= set(outcome[sure].tolist())
    assert {OUT_OF_GRID, OUT_OF_BAND, GATED, VALID} <= seen


def test_volume_association_edge_cases():
    """Planted volume features on a gentle ramp (|u| < 3 everywhere, |g|^2 = 0.0129), identity warp, float32-exact sample points
    (the identity warp returns them unchanged): a constant block (G = 0), a NaN voxel, an inf voxel; value_to_vox; determinism."""
    R = 32
    X, Y, Z = np.meshgrid(*(np.arange(R, dtype=np.float64),) * 3, indexing="ij")
    live = (0.1 * (X - 16) + 0.05 * (Y - 16) + 0.02 * (Z - 16)).astype(np.float32)
    live[4:8, 4:8, 4:8] = 0.25
    nan_v, inf_v = np.array([10, 11, 12]), np.array([20, 9, 14])
    live[tuple(nan_v)] = np.nan
    live[tuple(inf_v)] = np.inf
    off = np.stack(np.meshgrid(*((-1.5, -0.5, 0.5, 1.5),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    blk = 4.0 + np.stack(np.meshgrid(*((0.5, 1.25, 2.75),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(5)
    other = rng.uniform(0.0, 31.0, size=(300, 3)).astype(np.float32).astype(np.float64)
    pts = np.concatenate([nan_v + off, inf_v + off, blk, other])
    n_off, n_blk = len(off), len(blk)
    npos, nw = scene.fibonacci_nodes(12, R)
    sv = solve.WarpSolver(knn=4)
    sv.set_graph(npos, np.tile(IDENT, (12, 1)), nw)
    sv.set_samples(pts, np.tile([1.0, 0, 0], (len(pts), 1)), sort=False)
    live_t = torch.from_numpy(live).cuda()

    def run(vol, min_grad, value_to_vox=1.0):
        sv.associate_volume(vol, IDENT, band=4.0, max_dist=0.0, min_grad=min_grad, value_to_vox=value_to_vox)
        return sv.corr.clone(), sv.valid.clone()
    for min_grad in (0.05, 0.0):
        corr, valid = run(live_t, min_grad)
        v = valid.cpu().numpy().astype(bool)
        co, vo, outcome, _, _ = restate(pts, live, 1.0, 4.0, 0.0, min_grad)
        assert np.array_equal(v, vo)
        assert np.abs(corr.cpu().numpy() - co).max() <= 1e-9 and np.isfinite(corr.cpu().numpy()).all()
        # a cell touches a voxel iff the voxel is one of its corners: the 8 offsets of +-0.5 out of the 64
        touches = (np.abs(off) < 1.0).all(axis=1)
        assert touches.sum() == 8
        assert np.array_equal(v[:n_off], ~touches) and np.array_equal(v[n_off:2 * n_off], ~touches)
        # the constant block: G = 0 is never usable, min_grad = 0 included (t = s / G)
        assert not v[2 * n_off:2 * n_off + n_blk].any()
        assert (outcome[2 * n_off:2 * n_off + n_blk] == NO_GRADIENT).all()
        assert v[2 * n_off + n_blk:].sum() > 250
    # value_to_vox: halves scaled by 2 are the original values exactly -> the same bits
    ref = run(live_t, 0.05)
    got = run(torch.from_numpy(live * np.float32(0.5)).cuda(), 0.05, value_to_vox=2.0)
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])
    # determinism
    again = run(live_t, 0.05)
    assert torch.equal(ref[0], again[0]) and torch.equal(ref[1], again[1])
    # the Python layer's own refusals, with a solver that exists
    with pytest.raises(ValueError):
        sv.associate_volume(live_t[:, :, ::2], IDENT, band=4.0)
    with pytest.raises(ValueError):
        sv.associate_volume(live_t, IDENT, band=0.0)


def test_volume_loop_recovers_a_known_translation():
    """The scene of tests/test_gpu_configs.py::test_solve_recovers_a_known_translation (a static canonical sphere at 128^3 from three
    views, 256 nodes, band-2 samples; the live sphere translated by (0.6, -0.4, 0.3) voxel), the live frame given as the analytic
    TSDF of the translated sphere: iterate_volume, 2 rigid-mode steps + 10 iterations, against the existing depth-map loop
    (iterate_associated, same schedule and settings) on depth maps rendered from the same translated sphere.  Measure: rms of the
    restated live SDF (the trilinear value s) at the warped samples.  The volume loop's remaining rms must be no more than 1.25 x
    the depth loop's -- a margin for the different association (a Newton point against a ray hit), not for noise: both loops are
    deterministic.  The numbers are printed (and written to the directory $DFH_TEST_OUT names, if set) and committed as
    tests/golden/assoc_volume_recovery.json."""
    R, N, iters = 128, 256, 10
    rw, lm_abs, lm_rel, max_dist, huber, pcg_iters = 5.0, 10.0, 1e-2, 2.0, 0.5, 10
    angles = (0.0, 40.0, -40.0)
    H, W, fx, cx, cy = scene.CAMERAS["C2"]
    K = scene.intrinsics(fx, cx, cy); Kinv = np.linalg.inv(K)
    scale, center, tdist = scene.grid_params(R)
    T = torch.full((R, R, R), tdist, dtype=torch.float32, device="cuda")
    Wt = torch.zeros_like(T)
    lws = [scene.view_extrinsic(a) for a in angles]
    for lw in lws:
        d = torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)).cuda()
        kernels.integrate_depth(T, Wt, d, K, Kinv, lw, scale, center, tdist)
    fs = FrameSolver(K, scale, center, R / 2, knn=4, pcg_iters=pcg_iters, distributed=False)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    ident = np.tile(IDENT, (N, 1))
    fs.set_graph(node_pos, ident, node_w)
    S = fs.set_canonical(T, Wt, band=2.0)
    assert S > 10000
    truth = np.array([0.6, -0.4, 0.3])
    live = sphere_volume(R, R / 2 + truth, scene.SPHERE_R / scale).astype(np.float32)
    live_t = torch.from_numpy(live).cuda()
    depths = [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, sphere_offset=truth * scale)).cuda()
              for lw in lws]
    sv = fs.solver
    ident_t = torch.from_numpy(ident).cuda()

    def rms():
        xw, _ = solve.warp_points(sv.spos, None, IDENT, nbr=sv.snbr, node_dq=sv.node_dq, node_pos=sv.node_pos, node_w=sv.node_w)
        s = restate(xw.cpu().numpy(), live, band=np.inf, min_grad=0.0)[4]
        assert np.isfinite(s).all()
        return float(np.sqrt(np.mean(s * s)))
    before = rms()
    sv.iterate_associated(depths, K, Kinv, lws, scale, center, R / 2, IDENT, rw, max_dist, huber, lm_abs, lm_rel, n_iters=iters, n_global=2,
                          global_lm=0.1)
    _, n_depth = sv.cost()
    after_depth = rms()
    sv.node_dq.copy_(ident_t)
    sv.iterate_volume(live_t, IDENT, rw, 4.0, max_dist, huber, lm_abs, lm_rel, n_iters=iters, n_global=2, global_lm=0.1)
    _, n_volume = sv.cost()
    after_volume = rms()
    rec = {"workload": "128^3 static sphere from 3 views, 256 Fibonacci nodes, band-2 samples, live = the sphere translated by "
                       "(0.6, -0.4, 0.3) voxel; from the identity: 2 rigid-mode steps (lm 0.1) + 10 GN iterations: pcg_iters 10, huber 0.5, "
                       "rw 5, lm_abs 10, lm_rel 1e-2, max_dist 2; measure: rms of the trilinear live SDF at the warped samples, voxels",
           "samples": int(S), "rms_before": before, "rms_after_depth_loop_3_views": after_depth, "rms_after_volume_loop": after_volume,
           "valid_last_build_depth_loop": n_depth, "valid_last_build_volume_loop": n_volume}
    out_dir = os.environ.get("DFH_TEST_OUT")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        json.dump(rec, open(os.path.join(out_dir, "assoc_volume_recovery.json"), "w"), indent=1)
    print(json.dumps(rec))
    assert after_depth < before and n_volume > 0
    assert after_volume <= 1.25 * after_depth, rec


def test_frame_loop_with_the_volume_data_term():
    """SlabFrame at 64^3, three views, three frames: with data_term="volume" the loop stays finite, keeps valid samples in every
    frame and a warp field below one voxel; data_term="depth" is the loop without the argument, bit for bit."""
    R, N = 64, 96
    H, W, fx, cx, cy = scene.CAMERAS["C1"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    lws = [scene.view_extrinsic(a) for a in (0.0, 40.0, -40.0)]
    render = lambda off: [torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, sphere_offset=off)).cuda()
                          for lw in lws]
    first = render(None)
    frames = [render(np.array([0.4, -0.25, 0.15]) * np.sin(0.5 * (f + 1)) * scale) for f in range(3)]

    def run(**kw):
        sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=2.0, distributed=False)
        for d, lw in zip(first, lws):
            sf.integrate(d, lw)
        sf.refresh_samples()
        sv = sf.fs.solver
        counts, n_valid = [], []
        for ds in frames:
            counts.append(sf.step(ds, lws, gn_iters=6, on_updated=lambda: n_valid.append(sv.valid.sum()), **kw))
        torch.cuda.synchronize()
        return counts, [int(v) for v in n_valid], sv.node_dq.clone(), sf.T.clone(), sf.Wt.clone()
    counts, n_valid, dq, T, Wt = run(data_term="volume")
    print("volume data term: samples %s, valid in the last association %s" % (counts, n_valid))
    assert bool(torch.isfinite(T).all()) and bool(torch.isfinite(Wt).all()) and bool(torch.isfinite(dq).all())
    assert len(n_valid) == 3 and min(n_valid) > 0 and min(counts) > 0
    assert float(2 * dq[:, 4:].norm(dim=1).max()) < 1.0
    ref = run()
    got = run(data_term="depth")
    assert ref[0] == got[0] and ref[1] == got[1]
    assert torch.equal(ref[2], got[2]) and torch.equal(ref[3], got[3]) and torch.equal(ref[4], got[4])
    assert not torch.equal(ref[2], dq)                               # the volume term is another computation


def test_fusion_setup_correspondences_from_the_volume():
    """Fusion.setupCorrespondences(method='sdf') on the small ellipsoid pair of
    tests/test_gpu_solve.py::test_fusion_frame_loop_with_mesh_correspondences: correspondences on the live zero level set (restated
    trilinear value), most vertices kept, and solve(method='sdf') lowers the cost."""
    from dynamicfusion_body_amd import Fusion
    R = 40
    X, Y, Z = np.meshgrid(*(np.arange(R),) * 3, indexing="ij")
    sd = lambda c, r: np.clip(np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r, -3.0, 3.0).astype(np.float32)
    fu = Fusion(sd((19.6, 20.2, 19.9), 11.5), 3.0, subsample_rate=3.0, knn=4, marching_cubes_step_size=1, write_warpfield=False)
    fu._lw = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
    fu.initialize_canonical()
    nv0 = len(fu._vertices)
    live = sd((20.3, 19.8, 20.4), 11.7)                               # moved and slightly inflated
    mc_calls = []
    mc, fu.marching_cubes = fu.marching_cubes, lambda *a, **k: mc_calls.append(1) or mc(*a, **k)
    fu.setupCorrespondences(live, method='sdf', prune_result=True)
    assert not mc_calls                                               # no marching cubes of the live volume
    nv = len(fu._vertices)
    assert nv >= 0.8 * nv0 and len(fu._correspondences) == nv == len(fu._normals) == len(fu._neighbor_look_up)
    assert fu._faces is None
    s = restate(np.asarray(fu._correspondences), live, band=np.inf, min_grad=0.0)[4]
    print("kept %d of %d vertices; |live SDF| at the correspondences: max %.3g, median %.3g" % (nv, nv0, np.abs(s).max(), np.median(np.abs(s))))
    assert np.isfinite(s).all() and np.abs(s).max() <= 0.25
    for nd in fu._nodes:                                              # nodes re-anchored to their nearest kept vertex
        dist = np.linalg.norm(np.asarray(fu._vertices, dtype=np.float64) - nd[1], axis=1)
        assert 0 <= nd[0] < nv and dist[nd[0]] <= dist.min() + 1e-9
    fu.solve(method='sdf', precompute_lw=True, regularization_weight=1, iterations=8)
    assert 1 <= len(fu.last_costs) <= 3
    assert fu.last_costs[-1][-1] < fu.last_costs[0][0]
    assert len(fu._correspondences) == len(fu._vertices) > 0
