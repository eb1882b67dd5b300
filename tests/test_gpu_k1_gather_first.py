"""K1's gather-first column walk (integrate_depth_column_kernel with GATHER_FIRST: T and w loaded only for the packs the view
updates, the walk software-pipelined) against the row sweep (option k1_no_bricks) and the column walk that loads every pack
(k1_gather_first=0, k1_cull=0): the same T and w bit for bit, and the byte class dfh_integrate_depth_path reports for it."""
import numpy as np
import pytest
import torch

from dynamicfusion_body_amd import _lib, kernels, scene

pytestmark = pytest.mark.gpu

BENCH_ANGLES = (0.0, 30.0, -45.0, 60.0)          # bench.py's VIEW_ANGLES

# option sets: the new sweep (forced, so that small grids take it too) with every wave walking its whole share of its column
# (k1_nzi = 16: the pipelined loop body runs wherever a column has more than four bricks) and with one brick per wave (only the
# loop's prologue and tail), the row sweep, the walk over every pack
SWEEPS = {
    "gather_first": {"k1_bricks_min": 0, "k1_cull": 0, "k1_gather_first": 1, "k1_nzi": 16},
    "gather_first_one_brick": {"k1_bricks_min": 0, "k1_cull": 0, "k1_gather_first": 1, "k1_nzi": 1},
    "rows": {"k1_no_bricks": 1},
    "columns": {"k1_bricks_min": 0, "k1_cull": 0, "k1_gather_first": 0},
}


def set_options(opts):
    for name in ("k1_no_bricks", "k1_bricks_min", "k1_cull", "k1_gather_first", "k1_nzi"):
        _lib.set_option(name, opts.get(name))


def fuse(sweep, T0, W0, steps, K, scale, center, tdist, wmax, res=None, x_range=None, tsdf_res=None, extra=None):
    """T0, W0 (cloned) after the (lw, depth) steps on `sweep`."""
    set_options(dict(SWEEPS[sweep], **(extra or {})))
    try:
        T, Wt = T0.clone(), W0.clone()
        Kinv = np.linalg.inv(K)
        for lw, d in steps:
            kernels.integrate_depth(T, Wt, d, K, Kinv, lw, scale, center, tdist, wmax, tsdf_res=tsdf_res, res=res, x_range=x_range)
        torch.cuda.synchronize()
        return T, Wt
    finally:
        set_options({})


def assert_same(T0, W0, steps, K, scale, center, tdist, wmax, extra=None, **kw):
    outs = {s: fuse(s, T0, W0, steps, K, scale, center, tdist, wmax, extra=extra, **kw) for s in SWEEPS}
    for s in ("gather_first_one_brick", "rows", "columns"):
        assert torch.equal(outs["gather_first"][0], outs[s][0]), "T differs from the %s sweep" % s
        assert torch.equal(outs["gather_first"][1], outs[s][1]), "w differs from the %s sweep" % s
    return outs["gather_first"]


def bench_setup(R=256):
    H, W_, fx, cx, cy = scene.CAMERAS["C2"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    lws = [scene.view_extrinsic(a) for a in BENCH_ANGLES]
    depths = [torch.from_numpy(scene.render_depth(K, lw, H, W_, dtype=np.float32)).cuda() for lw in lws]
    return H, W_, K, scale, center, tdist, lws, depths


def test_bench_views_cycled_from_a_fresh_pair():
    R = 256
    H, W_, K, scale, center, tdist, lws, depths = bench_setup(R)
    T0 = torch.full((R, R, R), tdist, dtype=torch.float32, device="cuda")
    W0 = torch.zeros_like(T0)
    steps = [(lws[i % 4], depths[i % 4]) for i in range(20)]
    T, Wt = assert_same(T0, W0, steps, K, scale, center, tdist, 100.0)
    assert 0.3 < float((Wt > 0).float().mean()) < 0.9
    # the default (no options) takes the new sweep at 256^3 and gives the same bits
    Td, Wd = T0.clone(), W0.clone()
    for lw, d in steps:
        kernels.integrate_depth(Td, Wd, d, K, np.linalg.inv(K), lw, scale, center, tdist, 100.0)
    assert torch.equal(Td, T) and torch.equal(Wd, Wt)


@pytest.mark.parametrize("nzi", [2, 3, 5])
def test_walk_lengths_give_the_same_bits(nzi):
    """Waves walking 2, 3 and 5 bricks of their column (the last of them past the grid's ragged end): the same volumes."""
    res = (20, 45, 516)                                   # 17 bricks along z: 5 per wave
    H, W_, K, _, _, _, lws, depths = bench_setup()
    scale = scene.GRID_SIDE / max(res)
    center = scene.SPHERE_C.copy()
    tdist = 3.0 * scale
    T0 = torch.full(res, tdist, dtype=torch.float32, device="cuda")
    W0 = torch.zeros_like(T0)
    steps = [(lws[i % 4], depths[i % 4]) for i in range(6)]
    T, Wt = assert_same(T0, W0, steps, K, scale, center, tdist, 100.0, extra={"k1_nzi": nzi})
    assert int((Wt > 0).sum()) > 0


def test_random_prefilled_pair_and_the_weight_clamp():
    R = 256                                               # (two bricks per wave: the pipelined loop body runs)
    H, W_, K, _, _, _, lws, depths = bench_setup()
    scale, center, tdist = scene.grid_params(R)
    g = torch.Generator(device="cuda").manual_seed(5)
    T0 = (torch.rand((R, R, R), generator=g, device="cuda") * 2 - 1) * tdist
    W0 = torch.floor(torch.rand((R, R, R), generator=g, device="cuda") * 4)
    steps = [(lws[i % 4], depths[i % 4]) for i in range(6)]
    T, Wt = assert_same(T0, W0, steps, K, scale, center, tdist, 3.0)
    assert float(Wt.max()) == 3.0 and int((Wt == 3.0).sum()) > int((W0 == 3.0).sum())


def test_slab_that_cuts_bricks_and_a_ragged_grid():
    H, W_, K, _, _, _, lws, depths = bench_setup()
    # a slab of a 256^3 grid whose ends cut 4-plane bricks
    R = 256
    scale, center, tdist = scene.grid_params(R)
    a, b = 3, 202
    T0 = torch.full((b - a, R, R), tdist, dtype=torch.float32, device="cuda")
    W0 = torch.zeros_like(T0)
    steps = [(lws[i % 4], depths[i % 4]) for i in range(4)]
    assert_same(T0, W0, steps, K, scale, center, tdist, 100.0, res=(R, R, R), x_range=(a, b), tsdf_res=R)
    # Y odd, Z a multiple of 4 but not of 32 (bricks are 4 x 2 x 32)
    res = (50, 67, 292)
    scale = scene.GRID_SIDE / max(res)
    center = scene.SPHERE_C.copy()
    tdist = 3.0 * scale
    T0 = torch.full(res, tdist, dtype=torch.float32, device="cuda")
    W0 = torch.zeros_like(T0)
    T, Wt = assert_same(T0, W0, steps, K, scale, center, tdist, 100.0)
    assert int((Wt > 0).sum()) > 0


def test_non_pinhole_K_and_float64_depth():
    R = 256
    H, W_, fx, cx, cy = scene.CAMERAS["C2"]
    K = scene.intrinsics(fx, cx, cy)
    K[0, 1] = 0.37
    K[1, 1] = fx * 1.05
    scale, center, tdist = scene.grid_params(R)
    steps = []
    for i, a in enumerate(BENCH_ANGLES):
        lw = scene.view_extrinsic(a)
        d = scene.render_depth(K, lw, H, W_, dtype=np.float64)
        steps.append((lw, torch.from_numpy(d).cuda() if i % 2 == 0 else torch.from_numpy(d.astype(np.float32)).cuda()))
    T0 = torch.full((R, R, R), tdist, dtype=torch.float32, device="cuda")
    W0 = torch.zeros_like(T0)
    T, Wt = assert_same(T0, W0, steps, K, scale, center, tdist, 100.0)
    assert int((Wt > 0).sum()) > 0
    # pinhole K, float64 depth only
    K = scene.intrinsics(fx, cx, cy)
    steps = [(lw, torch.from_numpy(scene.render_depth(K, lw, H, W_, dtype=np.float64)).cuda()) for lw, _ in steps]
    assert_same(T0, W0, steps, K, scale, center, tdist, 100.0)


def test_nothing_everything_and_a_camera_inside_the_grid():
    R = 256
    H, W_, fx, cx, cy = scene.CAMERAS["C2"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    T0 = torch.full((R, R, R), tdist, dtype=torch.float32, device="cuda")
    W0 = torch.zeros_like(T0)
    lw0 = scene.view_extrinsic(0.0)
    # no valid depth anywhere: nothing is updated
    none = torch.zeros((H, W_), dtype=torch.float32, device="cuda")
    T, Wt = assert_same(T0, W0, [(lw0, none)], K, scale, center, tdist, 100.0)
    assert int((Wt > 0).sum()) == 0 and torch.equal(T, T0)
    # the grid wholly inside the frustum and in front of a wall at depth 8: every voxel is updated
    lw_all = lw0.copy()
    lw_all[2, 3] += 1.5
    far = torch.full((H, W_), -8.0, dtype=torch.float32, device="cuda")
    T, Wt = assert_same(T0, W0, [(lw_all, far)], K, scale, center, tdist, 100.0)
    assert int((Wt > 0).sum()) == Wt.numel()
    # camera inside the grid
    lw_in = lw0.copy()
    lw_in[2, 3] -= float(lw0[2, :3] @ center + lw0[2, 3]) - 0.013     # the grid's centre 13 mm in front of the camera
    d = torch.full((H, W_), -0.3, dtype=torch.float32, device="cuda")                 # a wall 0.3 m in front
    T, Wt = assert_same(T0, W0, [(lw_in, d), (lw0, d)], K, scale, center, tdist, 100.0)
    assert 0 < int((Wt > 0).sum()) < Wt.numel()


def test_culled_walk_forced_gather_first():
    """k1_gather_first=1 behind the culling passes (what 512^3 slabs take) gives the culled walk's bits."""
    R = 256
    H, W_, K, _, _, _, lws, depths = bench_setup()
    scale, center, tdist = scene.grid_params(R)
    T0 = torch.full((R, R, R), tdist, dtype=torch.float32, device="cuda")
    W0 = torch.zeros_like(T0)
    steps = [(lws[i % 4], depths[i % 4]) for i in range(5)]
    ref = fuse("rows", T0, W0, steps, K, scale, center, tdist, 100.0)
    for gf in (0, 1):
        T, Wt = fuse("columns", T0, W0, steps, K, scale, center, tdist, 100.0, extra={"k1_cull": 1, "k1_gather_first": gf, "k1_nzi": 16})
        assert torch.equal(T, ref[0]) and torch.equal(Wt, ref[1]), gf


def test_integrate_path_reports_the_byte_class():
    H, W_ = 480, 640
    depth = torch.zeros((H, W_), dtype=torch.float32)

    def path(res, dtype=torch.float32, x_range=None):
        T = torch.empty((1, 1, 1), dtype=dtype)
        return kernels.integrate_path(T, depth, res=res, x_range=x_range)

    set_options({})
    assert path((256, 256, 256)) == "rows"                       # the gather-first walk moves the row sweep's bytes
    assert path((512, 512, 512)) == "columns_culled"
    assert path((256, 256, 256), x_range=(0, 32)) == "rows"       # small slab: the row sweep itself
    assert path((256, 256, 256), dtype=torch.float64) == "exact"
    _lib.set_option("k1_gather_first", 0)
    try:
        assert path((256, 256, 256)) == "columns"
        assert path((512, 512, 512)) == "columns_culled"
        _lib.set_option("k1_gather_first", 1)
        assert path((512, 512, 512)) == "rows"
    finally:
        set_options({})
