"""GPU: the three fused layers of the volume data term -- dfh_gn_build_volume (the cell evaluation inside the data-row kernel),
dfh_gn_solve_volume (a frame's iterations in one call) and dfh_gn_global_sampled_volume (the rigid-mode step straight from the
samples) -- and the Python layers above them (WarpSolver.build_volume / iterate_volume / global_sampled_volume,
FrameSolver.global_iteration_volume(built=False), SlabFrame.step(data_term="volume", global_built=False)).

The scene is the one of tests/test_gpu_associate_volume.py (R = 32 sphere volume, 40 Fibonacci nodes with random twists, a
non-identity lw, ray samples whose first 200 lie anywhere in [-2, 33]^3), with the solver's SORTED samples: S = 4000 is 31 full
tiles plus one of 32 samples, S = 421 three tiles plus 37 samples, S = 128 exactly one tile."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gn_np as G
from oracle import oracle_np as O
from dynamicfusion_body_amd import _lib, scene, solve
from dynamicfusion_body_amd.device import current_stream_ptr
from dynamicfusion_body_amd.pipeline import SlabFrame
from test_gpu_associate_volume import ray_samples, restate, sphere_scene

pytestmark = pytest.mark.gpu


def make_solver(k, S, dtype=np.float32):
    """(solver with the scene's graph -- regulariser table included -- and S sorted samples, live volume on the device and on
    the host, scene)."""
    sc = sphere_scene()
    pts, d = ray_samples(max(S, 200), sc)                             # (the generator plants 200 points: fewer = the first S of them)
    pts, d = pts[:S], d[:S]
    sv = solve.WarpSolver(knn=k, pcg_iters=10)
    node_nbr, _ = solve.sample_knn(sc["npos"], sc["npos"], sc["nw"], k)
    sv.set_graph(sc["npos"], sc["ndq"], sc["nw"], node_nbr=node_nbr)
    sv.set_samples(pts, d)
    assert sv.S == S and int(sv.lib.dfh_gn_tile_samples()) == 128
    live = sc["live"].astype(dtype)
    return sv, torch.from_numpy(live).cuda(), live, sc


def reset(sv, sc):
    sv.node_dq.copy_(torch.from_numpy(sc["ndq"]).cuda())


# (band, max_dist, huber, rw)
SETTINGS = [(4.0, 0.0, 0.0, 0.0), (4.0, 2.0, 0.5, 5.0), (1e-3, 2.0, 0.5, 5.0)]


@pytest.mark.parametrize("k,S", [(1, 421), (3, 421), (4, 421), (8, 421), (4, 128), (4, 4000)])
def test_fused_volume_build_equals_associate_then_build(k, S):
    """build_volume (one launch sequence, dfh_gn_build_volume) against associate_volume + build: corr, valid and the system
    {J^T J | J^T r | cost, count}, bit for bit, over poisoned outputs."""
    sv, live_t, _, sc = make_solver(k, S)
    for band, max_dist, huber, rw in SETTINGS:
        sv.associate_volume(live_t, sc["lw"], band, max_dist, min_grad=0.5)
        sv.build(sc["lw"], rw, huber)
        corr, valid, system = sv.corr.clone(), sv.valid.clone(), sv.system.clone()
        sv.corr.fill_(7.0)
        sv.valid.fill_(3)
        sv.system.fill_(float("nan"))
        sv.build_volume(live_t, sc["lw"], rw, band, max_dist, huber, min_grad=0.5)
        n_valid = int(valid.sum())
        print("knn %d S %d band %g max_dist %g huber %g rw %g: %d valid, count %g" % (k, S, band, max_dist, huber, rw, n_valid,
                                                                                    float(sv.cost_count[1])))
        assert torch.equal(sv.corr, corr) and torch.equal(sv.valid, valid)
        assert bool(torch.isfinite(system).all()) and torch.equal(sv.system, system)
        assert float(sv.cost_count[1]) == n_valid
        if band == 4.0:
            assert 0 < n_valid < S                                    # both outcomes occur
        else:
            assert n_valid == 0                                       # every tile takes the dead-tile exit


def test_one_call_volume_solve_equals_separate_calls():
    """iterate_volume -- one dfh_gn_solve_volume call -- against the three older sequences the options select: the association as
    a launch of its own, a library call per build and per solve, one call per iteration.  Everything they leave is bit-identical."""
    sv, live_t, _, sc = make_solver(4, 4000)
    start = torch.from_numpy(sc["ndq"]).cuda()
    runs = {}
    for option in (None, "py_gn_no_fused_assoc", "py_gn_no_fused_iter", "py_gn_iter_per_call"):
        _lib.reset_options()
        if option:
            _lib.set_option(option, 1)
        reset(sv, sc)
        sv.iterate_volume(live_t, sc["lw"], 5.0, 4.0, max_dist=2.0, huber=0.5, lm_abs=10.0, lm_rel=1e-2, n_iters=3, n_global=2,
                          global_lm=0.1)
        sv.check_status()
        runs[option] = [t.clone() for t in (sv.node_dq, sv.dx, sv.corr, sv.valid, sv.system)]
    _lib.reset_options()
    ref = runs[None]
    assert bool(torch.isfinite(ref[0]).all()) and not torch.equal(ref[0], start)
    assert int(ref[3].sum()) > 0
    for option, got in runs.items():
        for name, a, b in zip(("node_dq", "dx", "corr", "valid", "system"), ref, got):
            assert torch.equal(a, b), (option, name)


def host_arrays(sv):
    return sv.spos.cpu().numpy(), sv.snrm.cpu().numpy(), sv.snbr.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("k", [1, 3, 4, 8])
def test_sampled_volume_step_vs_oracle(k, dtype, stride):
    """dfh_gn_global_sampled_volume against oracle/gn_np.global_step_sampled with the restated cell evaluation as its
    association: valid count exact, twist and node DQs to 1e-9 (the bound of the depth version's test,
    tests/test_gpu_configs.py::test_rigid_mode_step_variants_and_oracle).  No sample is left out: every decision of the
    restatement must be further than 1e-6 from flipping, or the test fails."""
    sv, live_t, live, sc = make_solver(k, 4000, dtype)
    pos, nrm, nbr = host_arrays(sv)
    warped = O.warp(pos, sc["ndq"][nbr], sc["npos"][nbr], sc["nw"][nbr], m_lw=sc["lw"])
    margin = restate(warped, live, 1.0, 4.0, 2.0, 0.5)[3]
    print("knn %d %s stride %d: smallest margin %.3g" % (k, np.dtype(dtype).name, stride, margin.min()))
    assert margin.min() > 1e-6
    associate = lambda xw: restate(xw, live, 1.0, 4.0, 2.0, 0.5)[:2]
    dq_o, xi_o, n_o = G.global_step_sampled(sc["ndq"], pos, nrm, nbr, sc["npos"], sc["nw"], sc["lw"], associate, 0.5, 0.1, stride=stride,
                                            tile=int(sv.lib.dfh_gn_tile_samples()))
    sv.global_sampled_volume(live_t, sc["lw"], 4.0, max_dist=2.0, huber=0.5, lm_rel=0.1, n_steps=1, stride=stride, min_grad=0.5)
    xi = sv.global_xi.cpu().numpy()
    print("valid %d (oracle %d), max |xi - oracle| %.3g, max |dq - oracle| %.3g" % (
        int(xi[7]), n_o, np.abs(xi[:6] - xi_o).max(), np.abs(sv.node_dq.cpu().numpy() - dq_o).max()))
    assert int(xi[7]) == n_o and n_o > 100
    assert np.abs(xi[:6] - xi_o).max() <= 1e-9
    assert np.abs(sv.node_dq.cpu().numpy() - dq_o).max() <= 1e-9


def test_sampled_volume_step_variants():
    sv, live_t, _, sc = make_solver(4, 4000)
    lw = sc["lw"]
    step = lambda n, stride=4, band=4.0: sv.global_sampled_volume(live_t, lw, band, max_dist=2.0, huber=0.5, lm_rel=0.1, n_steps=n,
                                                                   stride=stride, min_grad=0.5)
    # two steps in one call = two calls of one step
    reset(sv, sc)
    step(2)
    two = (sv.node_dq.clone(), sv.global_xi.clone())
    reset(sv, sc)
    step(1)
    one = (sv.node_dq.clone(), sv.global_xi.clone())
    step(1)
    assert torch.equal(sv.node_dq, two[0]) and torch.equal(sv.global_xi, two[1])
    assert float(two[1][7]) > 100 and not torch.equal(one[0], two[0])
    # the sharded form: the 29 sums, then dfh_gn_global_apply
    reset(sv, sc)
    sums = torch.zeros(32, dtype=torch.float64, device="cuda")
    xi = torch.zeros(8, dtype=torch.float64, device="cuda")
    term = sv._volume_term(live_t, 4.0, 2.0, 0.5, 1.0)
    _lib.check(sv.lib.dfh_gn_global_sampled_volume(sv._problem(lw, huber=0.5), term, 4, 0.1, 1, 0, sums.data_ptr(), sv._gs_ws.data_ptr(),
                                                   sv._gs_ws.numel() * 8, current_stream_ptr()), "dfh_gn_global_sampled_volume")
    assert torch.equal(sv.node_dq, torch.from_numpy(sc["ndq"]).cuda())          # (nothing applied yet)
    _lib.check(sv.lib.dfh_gn_global_apply(sums.data_ptr(), 0.1, sv.N, sv.node_dq.data_ptr(), xi.data_ptr(), current_stream_ptr()),
               "dfh_gn_global_apply")
    assert torch.equal(sv.node_dq, one[0]) and torch.equal(xi, one[1])
    # every tile, no regulariser: the built system holds the same sums
    reset(sv, sc)
    step(1, stride=1)
    xi_s = sv.global_xi.cpu().numpy()[:6].copy()
    dq_s = sv.node_dq.clone()
    reset(sv, sc)
    sv.iterate_volume(live_t, lw, 0.0, 4.0, max_dist=2.0, huber=0.5, n_iters=0, n_global=1, global_lm=0.1, min_grad=0.5)
    xi_b = sv.global_xi.cpu().numpy()[:6]
    print("sampled %s\nbuilt   %s" % (xi_s, xi_b))
    assert np.abs(xi_s).max() > 1e-3
    assert np.abs(xi_s - xi_b).max() <= 1e-9
    assert float((sv.node_dq - dq_s).abs().max()) <= 1e-9
    # nothing inside the band: no valid sample, no step
    reset(sv, sc)
    step(1, band=1e-3)
    xi0 = sv.global_xi.cpu().numpy()
    assert xi0[7] == 0.0 and np.all(xi0[:6] == 0.0)
    assert torch.equal(sv.node_dq, torch.from_numpy(sc["ndq"]).cuda())


def test_frame_loop_volume_paths():
    """SlabFrame at 64^3, three views, three frames (the shapes of tests/test_gpu_associate_volume.py::
    test_frame_loop_with_the_volume_data_term): the default volume loop -- fused build, one call per solve -- leaves what the
    loop with the association as a launch of its own leaves, bit for bit; with global_built=False the rigid-mode steps come from
    the samples: another computation, finite, with valid samples in every frame and a warp field below one voxel."""
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

    def run(option=None, **kw):
        _lib.reset_options()
        if option:
            _lib.set_option(option, 1)
        sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=2.0, distributed=False)
        for d, lw in zip(first, lws):
            sf.integrate(d, lw)
        sf.refresh_samples()
        sv = sf.fs.solver
        counts, n_valid = [], []
        for ds in frames:
            counts.append(sf.step(ds, lws, gn_iters=6, on_updated=lambda: n_valid.append(sv.valid.sum()), data_term="volume", **kw))
        torch.cuda.synchronize()
        _lib.reset_options()
        return counts, [int(v) for v in n_valid], sv.node_dq.clone(), sf.T.clone(), sf.Wt.clone()
    ref = run()
    old = run("py_gn_no_fused_assoc")
    assert ref[0] == old[0] and ref[1] == old[1]
    assert torch.equal(ref[2], old[2]) and torch.equal(ref[3], old[3]) and torch.equal(ref[4], old[4])
    assert torch.equal(run(global_built=True)[2], ref[2])              # (None is the built step for volumes)
    counts, n_valid, dq, T, Wt = run(global_built=False)
    print("sampled rigid-mode steps: samples %s, valid in the last association %s, largest translation %.3g" % (
        counts, n_valid, float(2 * dq[:, 4:].norm(dim=1).max())))
    assert bool(torch.isfinite(T).all()) and bool(torch.isfinite(Wt).all()) and bool(torch.isfinite(dq).all())
    assert len(n_valid) == 3 and min(n_valid) > 0 and min(counts) > 0
    assert float(2 * dq[:, 4:].norm(dim=1).max()) < 1.0
    assert not torch.equal(dq, ref[2])
