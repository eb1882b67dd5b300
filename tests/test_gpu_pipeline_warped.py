"""GPU: the frame loop with the depth-driven canonical update (SlabFrame.step(update="depth"): K1w,
kernels.integrate_depth_dqb in place of the live volume + fuse_volume_dqb) on 32^3, 64 nodes, two views, three frames of the
scene's moving sphere."""
import numpy as np
import pytest
import torch

from dynamicfusion_body_amd import kernels, scene
from dynamicfusion_body_amd.pipeline import SlabFrame

pytestmark = pytest.mark.gpu

R, N = 32, 64
ANGLES = (0.0, 40.0)


def frames(n=3):
    H, W, fx, cx, cy = scene.CAMERAS["C1"]
    K = scene.intrinsics(fx, cx, cy)
    scale = scene.grid_params(R)[0]
    lws = [scene.view_extrinsic(a) for a in ANGLES]
    out = []
    for f in range(n + 1):                          # frame 0 builds the canonical volume
        off = np.array([0.4, -0.25, 0.15]) * np.sin(0.5 * f) * scale
        out.append([torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, sphere_offset=off)).cuda() for lw in lws])
    return K, lws, out


def new_loop(K, lws, first):
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=2.0, distributed=False)
    for d, lw in zip(first, lws):
        sf.integrate(d, lw)
    assert sf.refresh_samples() > 100
    return sf


@pytest.fixture(scope="module")
def inputs():
    return frames()


def test_depth_route_needs_no_live_volume(inputs):
    K, lws, fr = inputs
    sf = new_loop(K, lws, fr[0])
    sf.live.fill_(float("nan"))
    sf.live_w.fill_(float("nan"))
    for ds in fr[1:]:
        n = sf.step(ds, lws, gn_iters=4, update="depth", data_term="depth", relax=1.0)
        assert n > 100
    torch.cuda.synchronize()
    assert bool(torch.isnan(sf.live).all()) and bool(torch.isnan(sf.live_w).all())
    assert bool(torch.isfinite(sf.T).all()) and bool(torch.isfinite(sf.Wt).all())
    assert bool(torch.isfinite(sf.fs.solver.node_dq).all())
    # the stages keep their names, and the volume data term still sweeps the live volume for its solve
    ms = {}
    assert sf.step(fr[1], lws, gn_iters=2, update="depth", data_term="volume", stage_ms=ms) > 100
    assert sorted(ms) == ["allgather", "live_tsdf", "samples", "solve", "tsdf_update"]
    assert bool(torch.isfinite(sf.live).all()) and bool(torch.isfinite(sf.T).all())


@pytest.mark.parametrize("weight", ["node_distance", "unit"])
def test_one_frame_is_one_kernel_call(inputs, weight):
    K, lws, fr = inputs
    sf = new_loop(K, lws, fr[0])
    sf.step(fr[1], lws, gn_iters=4, update="depth", update_weight=weight)          # (first frame: stores the neighbourhoods)
    T0, W0 = sf.T.clone(), sf.Wt.clone()
    called = []
    sf.step(fr[2], lws, gn_iters=4, update="depth", update_weight=weight, relax=1.0, on_updated=lambda: called.append(1))
    assert called == [1]
    sv = sf.fs.solver
    kernels.integrate_depth_dqb(T0, W0, fr[2], sf.K, sf.Kinv, lws, sf.scale, sf.center, sf.tdist_world, sv.node_pos, sv.node_dq,
                                sv.node_w, 4, sf.ident_lw, weight=weight, tsdf_res=R)
    assert bool((W0 != 0).any()) and not torch.equal(sv.node_dq, torch.tensor(sf.ident_lw, device="cuda").expand(N, 8))
    assert torch.equal(sf.T, T0) and torch.equal(sf.Wt, W0)


def test_volume_route_is_unchanged_and_bad_values_raise(inputs):
    K, lws, fr = inputs
    a, b = new_loop(K, lws, fr[0]), new_loop(K, lws, fr[0])
    for ds in fr[1:]:
        na = a.step(ds, lws, gn_iters=4)
        nb = b.step(ds, lws, gn_iters=4, update="volume", update_weight="node_distance")
        assert na == nb
    assert torch.equal(a.T, b.T) and torch.equal(a.Wt, b.Wt) and torch.equal(a.fs.solver.node_dq, b.fs.solver.node_dq)
    assert torch.equal(a.live, b.live)
    T0 = a.T.clone()
    with pytest.raises(ValueError, match="update must be"):
        a.step(fr[1], lws, update="live")
    with pytest.raises(ValueError, match="update_weight must be"):
        a.step(fr[1], lws, update="depth", update_weight="mean")
    assert torch.equal(a.T, T0)
