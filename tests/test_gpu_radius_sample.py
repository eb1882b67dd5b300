"""GPU: the radius subsampling on the device (dfh_radius_sample, graph.uniform_sample_device) against the host loop
graph.uniform_sample on the same fp64 input -- "equal" is np.array_equal on the index list, and the sample positions are the
input rows -- and the layers above it: graph.*_graph_device(sampler="device"), Fusion.graph_sampler, SlabFrame.construct_graph /
update_graph(sampler="device")."""
import ctypes

import numpy as np
import pytest
import torch

from dynamicfusion_body_amd import Fusion, _lib, graph, scene
from dynamicfusion_body_amd.pipeline import SlabFrame

pytestmark = pytest.mark.gpu


def _raw(points, radius, capacity=None):
    """dfh_radius_sample itself -> (idx written (numpy), count, rounds, workspace bytes)."""
    lib = _lib.load()
    P = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float64)).cuda()
    n = P.shape[0]
    cap = n if capacity is None else capacity
    nbytes = lib.dfh_radius_sample_workspace_bytes(n)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device="cuda")
    idx = torch.full((cap + 8,), -1, dtype=torch.int32, device="cuda")          # (8 guard words behind the capacity)
    count, rounds = ctypes.c_long(-1), ctypes.c_int(-1)
    _lib.check(lib.dfh_radius_sample(P.data_ptr(), n, float(radius), idx.data_ptr(), cap, ctypes.byref(count), ctypes.byref(rounds),
                                     ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream), "dfh_radius_sample")
    out = idx.cpu().numpy()
    assert (out[cap:] == -1).all()                                              # nothing written past the capacity
    return out[:min(cap, count.value)], count.value, rounds.value, nbytes


def _equal_to_host(points, radius):
    """uniform_sample_device == uniform_sample on the fp64 input; returns the index list."""
    p64 = np.array(points, dtype=np.float64)
    want_v, want_i = graph.uniform_sample(p64, radius)
    got_v, got_i = graph.uniform_sample_device(points, radius)
    assert got_v.is_cuda and got_v.dtype == torch.float64 and got_i.is_cuda and got_i.dtype == torch.int32
    gi = got_i.cpu().numpy()
    assert np.array_equal(gi, np.asarray(want_i, dtype=np.int64)), (len(gi), len(want_i))
    assert np.array_equal(got_v.cpu().numpy(), p64[gi]) and np.array_equal(p64[gi], np.asarray(want_v).reshape(-1, 3))
    return gi


def _shell64():
    """Voxel centres with |d| < 1 of a sphere of radius 20 about the centre of a 64^3 grid, x-major: 10 256 points."""
    g = np.stack(np.meshgrid(*[np.arange(64.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    d = np.linalg.norm(g - 31.5, axis=1) - 20.0
    return np.ascontiguousarray(g[np.abs(d) < 1.0])


def _cloud():
    return np.random.default_rng(11).uniform(0.0, 20.0, size=(5000, 3))


# ---- 1. golden g8 ------------------------------------------------------------------------------------------------------------
def test_golden_g8_indices(golden):
    g = golden("g8_graph_io")
    v, i = graph.uniform_sample_device(g["verts"], float(g["radius"]))
    assert np.array_equal(i.cpu().numpy(), g["cg_idx"]) and np.array_equal(i.cpu().numpy(), g["us_i"])
    assert np.array_equal(v.cpu().numpy(), g["us_v"])


def test_fusion_with_the_device_sampler_matches_the_reference(golden):
    """Every assertion of test_gpu_graph.py::test_construct_and_update_graph_device_match_reference, graph_sampler="device"."""
    g = golden("g8_graph_io")
    k = int(g["knn"])
    fu = Fusion(np.zeros((4, 4, 4)), 1.0, knn=k, write_warpfield=False)
    fu.graph_sampler = "device"
    fu._vertices, fu._radius = g["verts"], float(g["radius"])
    fu.construct_graph()
    assert np.array_equal(np.array([n[0] for n in fu._nodes]), g["cg_idx"])
    assert np.array_equal(np.array([n[1] for n in fu._nodes]), g["cg_pos"])
    assert np.array_equal(np.array([n[2] for n in fu._nodes]), g["cg_dq"]) and fu._nodes[0][2].dtype == np.float32
    assert np.array_equal(np.array([n[3] for n in fu._nodes]), g["cg_w"])
    assert np.array_equal(np.asarray(fu._neighbor_look_up), g["cg_lookup"])
    fu._nodes = [(n[0], n[1], g["ug_dq_in"][i], n[3]) for i, n in enumerate(fu._nodes)]
    fu._vertices = g["verts2"]
    n_new = fu.update_graph(refresh_surface=False)
    assert n_new == len(g["ug_idx"]) - len(g["cg_idx"]) and n_new > 0
    assert np.array_equal(np.array([n[0] for n in fu._nodes]), g["ug_idx"])
    assert np.array_equal(np.array([n[1] for n in fu._nodes]), g["ug_pos"])
    assert np.abs(np.array([np.asarray(n[2], dtype=np.float64) for n in fu._nodes]) - g["ug_dq"]).max() <= 1e-12   # device exp vs libm
    assert np.array_equal(np.array([n[3] for n in fu._nodes]), g["ug_w"])
    assert np.array_equal(np.asarray(fu._neighbor_look_up), g["ug_lookup"])
    assert fu._curr_tsdf is None and fu._correspondences == []


# ---- 2. the 64^3 shell: several rounds, many cells -----------------------------------------------------------------------------
def test_shell_64_in_voxel_order_and_permuted():
    p = _shell64()
    assert p.shape == (10256, 3)
    gi = _equal_to_host(p, 6.0)
    assert len(gi) == 130
    _, count, rounds, _ = _raw(p, 6.0)
    assert count == 130 and 2 <= rounds <= 130                         # several rounds, at most one per node
    perm = np.random.default_rng(5).permutation(len(p))
    gp = _equal_to_host(p[perm], 6.0)
    assert not np.array_equal(np.sort(perm[gp]), gi)                    # another order, another set


# ---- 3. a chain: the dependency chain is as long as the output ------------------------------------------------------------------
def test_chain_runs_one_round_per_node():
    p = np.zeros((200, 3))
    p[:, 0] = 0.6 * np.arange(200)
    gi = _equal_to_host(p, 1.0)
    assert np.array_equal(gi, np.arange(0, 200, 2))
    idx, count, rounds, _ = _raw(p, 1.0)
    assert count == 100 and np.array_equal(idx, gi)
    assert 100 <= rounds <= 200


# ---- 4. exact ties ---------------------------------------------------------------------------------------------------------------
def test_integer_lattice_with_duplicates_and_exact_ties():
    p = np.random.default_rng(7).integers(0, 6, size=(3000, 3)).astype(np.float64)
    d = np.linalg.norm(p[:200, None] - p[None, :200], axis=2)
    assert (d == 2.0).any() and (d + np.eye(200) == 0.0).any()         # distances equal to the radius, and duplicates
    gi = _equal_to_host(p, 2.0)
    assert 8 <= len(gi) <= 64


def test_3_4_12_pair_at_and_just_below_the_radius():
    p = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 12.0]])
    assert np.array_equal(_equal_to_host(p, 13.0), [0, 1])              # dist == radius: kept (strict comparison)
    assert np.array_equal(_equal_to_host(p, np.nextafter(13.0, np.inf)), [0])


def test_uniform_cloud():
    gi = _equal_to_host(_cloud(), 1.5)
    assert 900 <= len(gi) <= 1300


def test_more_blocks_than_one_round_of_the_output_scan():
    """The output's count / scan / emit counts 256 points a block and scans 1 024 blocks a round: 1 026 blocks here.  The points
    are runs of identical points at 150 sites far apart, so the selection is the first point of every run: indices in blocks on
    both sides of the round's edge (and of every wave's edge), most blocks empty, and only 150 steps of the host loop."""
    rng = np.random.default_rng(31)
    n, sites = 1024 * 256 + 300, 150
    starts = np.concatenate([[0], np.sort(rng.choice(np.arange(1, n - 300), size=sites - 2, replace=False)), [n - 7]])
    site_pos = 10.0 * np.stack(np.unravel_index(rng.permutation(216)[:sites], (6, 6, 6)), -1)
    p = np.repeat(site_pos, np.diff(np.concatenate([starts, [n]])), axis=0)
    assert p.shape == (n, 3) and (starts >= 1024 * 256).any()
    gi = _equal_to_host(p, 1.0)
    assert np.array_equal(gi, starts)
    idx, count, rounds, _ = _raw(p, 1.0)
    assert count == sites and np.array_equal(idx, starts)


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------
def test_one_point_and_identical_points():
    assert np.array_equal(_equal_to_host(np.array([[1.5, -2.0, 3.0]]), 0.7), [0])
    assert np.array_equal(_equal_to_host(np.tile([[0.3, 0.1, -4.0]], (500, 1)), 0.25), [0])


def test_radius_below_every_gap_and_a_small_capacity():
    p = np.stack(np.meshgrid(np.arange(10.0), np.arange(6.0), np.arange(5.0), indexing="ij"), -1).reshape(-1, 3)
    p = p[np.random.default_rng(2).permutation(300)]
    assert np.array_equal(_equal_to_host(p, 0.999), np.arange(300))     # every gap is >= 1
    assert np.array_equal(_equal_to_host(p, 1.0), np.arange(300))       # ... and a gap equal to the radius keeps both
    idx, count, _, _ = _raw(p, 0.999, capacity=100)
    assert count == 300 and np.array_equal(idx, np.arange(100))


def test_radius_above_the_whole_extent():
    assert np.array_equal(_equal_to_host(_cloud()[:700], 40.0), [0])


def test_far_outlier_costs_rounds_not_memory():
    c = _cloud()
    p = np.concatenate([c[:2500], [[1e6, 1e6, 1e6]], c[2500:]])
    gi = _equal_to_host(p, 1.5)
    assert 2500 in gi
    near = np.concatenate([c[:2500], [[10.0, 10.0, 10.0]], c[2500:]])   # as many points, no outlier
    idx, count, rounds, nbytes = _raw(p, 1.5)                           # (run in exactly the workspace the size query gives)
    _, _, rounds_near, nbytes_near = _raw(near, 1.5)
    assert count == len(gi) and np.array_equal(idx, gi)
    assert nbytes == nbytes_near                                        # a function of the count alone
    assert rounds > rounds_near                                         # the outlier's price: larger cells, more rounds


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_pair_across_a_cell_boundary(axis):
    """Cells are a shade wider than the radius (side = radius (1 + 2^-20), first cell from the lowest coordinate 0): a = 1 lies in
    cell 0, b = a + (1 - 2^-52) = 2 - 2^-52 in cell 1, their difference is exactly radius (1 - 2^-52) < radius: a rejects b only
    if the search covers the neighbouring cell.  The first point pins the box's corner and is at distance exactly 1 from a."""
    r = 1.0
    e = np.zeros(3)
    e[axis] = 1.0
    a, b = 1.0 * e, (2.0 - 2.0 ** -52) * e
    assert (b - a)[axis] == r * (1 - 2.0 ** -52)
    for scale in (1.0, 3.0, 0.1):                                       # (other radii: other roundings of the side)
        p = np.array([0 * e, a, b, b + 5 * e]) * scale
        gi = _equal_to_host(p, r * scale)
        if scale == 1.0:
            assert np.array_equal(gi, [0, 1, 3]), gi
    # the same gap wherever the boundary falls: a sweep of offsets over two cells
    t = np.linspace(0.0, 2.0, 65)
    for t0 in t:
        p = np.array([0 * e, (1.0 + t0) * e, (1.0 + t0) * e + (1 - 2.0 ** -52) * e])
        want = graph.uniform_sample(p, r)[1]
        got = graph.uniform_sample_device(p, r)[1].cpu().numpy()
        assert np.array_equal(got, want), (t0, got, want)


# ---- 6. inputs -----------------------------------------------------------------------------------------------------------------
def test_input_kinds_agree_and_nan_is_refused():
    p32 = _cloud()[:1200].astype(np.float32)
    want = _equal_to_host(p32, 1.5)                                     # float32 numpy (compared on its fp64 conversion)
    wide = torch.from_numpy(np.concatenate([p32, -p32], axis=1).astype(np.float64))
    view = wide[:, :3]
    assert not view.is_contiguous()
    assert np.array_equal(graph.uniform_sample_device(view, 1.5)[1].cpu().numpy(), want)
    cuda = torch.from_numpy(p32.astype(np.float64)).cuda()
    assert np.array_equal(graph.uniform_sample_device(cuda, 1.5)[1].cpu().numpy(), want)
    bad = p32.astype(np.float64)
    bad[17, 1] = np.nan
    with pytest.raises(ValueError):
        graph.uniform_sample_device(bad, 1.5)
    with pytest.raises(ValueError):
        graph.uniform_sample_device(p32, 0.0)


# ---- 7. update_graph_device(sampler="device") against sampler="host" -----------------------------------------------------------
@pytest.mark.parametrize("gathered", [False, True])
def test_update_graph_device_samplers_agree(golden, gathered):
    g = golden("g8_graph_io")
    k = int(g["knn"])
    chunk = g["verts"][::7] + np.array([9.0, 0.0, 0.0])                 # a second rank's unsupported points
    seen = []

    def gather_host(u):
        seen.append(type(u))
        return np.concatenate([u, chunk])

    def gather_device(u):
        seen.append(type(u))
        assert u.is_cuda
        return torch.cat([u, torch.from_numpy(chunk).cuda()])
    args = (g["cg_pos"], g["ug_dq_in"], g["cg_w"], g["verts2"], float(g["radius"]), k)
    host = graph.update_graph_device(*args, gather_unsupported=gather_host if gathered else None, sampler="host")
    dev = graph.update_graph_device(*args, gather_unsupported=gather_device if gathered else None, sampler="device")
    assert host[5] == dev[5] and host[5] > 0
    for a, b in zip(host[:5], dev[:5]):
        assert a.dtype == b.dtype and torch.equal(a, b)
    if gathered:
        assert seen == [np.ndarray, torch.Tensor]


# ---- 8. the loop, R = 64, one rank -----------------------------------------------------------------------------------------------
R = 64


def _scene():
    H, W, fx, cx, cy = scene.CAMERAS["C2"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    lws = [scene.view_extrinsic(a) for a in (0.0, 40.0)]
    depth = lambda lw, off=None: torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, sphere_offset=off)).cuda()
    return K, scale, center, tdist, lws, depth


def _frame(K, scale, center, tdist, node_pos, node_w):
    return SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=2.0, distributed=False)


def test_slab_frame_builds_its_own_graph():
    K, scale, center, tdist, lws, depth = _scene()
    radius = 5.0
    first = [depth(lw) for lw in lws]
    sf = _frame(K, scale, center, tdist, None, None)
    for d, lw in zip(first, lws):
        sf.integrate(d, lw)
    with pytest.raises(ValueError):
        sf.step(first, lws)
    with pytest.raises(ValueError):
        sf.update_graph()
    pts, nrm = sf.band_samples()                                        # the bare extraction works without a graph
    assert pts.shape[0] > 1000 and nrm.shape == pts.shape
    p = pts.cpu().numpy()
    p = p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))]
    want, _ = graph.uniform_sample(p, radius)
    N = sf.construct_graph(radius)
    sv = sf.fs.solver
    assert N == len(want) == sv.N and N > 20
    assert np.array_equal(sv.node_pos.cpu().numpy(), want)
    assert torch.equal(sv.node_w, torch.full((N,), 2 * radius, dtype=torch.float64, device="cuda"))
    assert sv.S == pts.shape[0]
    assert int(graph.unsupported_vertices(sv.spos, sv.snbr, sv.node_pos, sv.node_w).sum()) == 0      # every band sample is supported
    # a second frame that is handed the host result from outside: the same loop, bit for bit
    sh = _frame(K, scale, center, tdist, want, np.full(N, 2 * radius))
    for d, lw in zip(first, lws):
        sh.integrate(d, lw)
    sh.refresh_samples()
    amp = np.array([0.5, -0.3, 0.2])
    for f in range(3):
        off = amp * np.sin(0.3 * (f + 1)) * scale
        ds = [depth(lw, off) for lw in lws]
        n1 = sf.step(ds, lws, gn_iters=10)
        n2 = sh.step(ds, lws, gn_iters=10)
        assert n1 == n2 > 1000
    assert torch.equal(sf.T, sh.T) and torch.equal(sf.Wt, sh.Wt)
    assert torch.equal(sf.fs.solver.node_dq, sh.fs.solver.node_dq)
    assert bool(torch.isfinite(sf.fs.solver.node_dq).all())
    assert int(graph.unsupported_vertices(sv.spos, sv.snbr, sv.node_pos, sv.node_w).sum()) == 0
    # sampler="host" builds the same graph
    s2 = _frame(K, scale, center, tdist, None, None)
    for d, lw in zip(first, lws):
        s2.integrate(d, lw)
    assert s2.construct_graph(radius, sampler="host") == N
    assert np.array_equal(s2.fs.solver.node_pos.cpu().numpy(), want)


def test_slab_frame_update_graph_samplers_insert_the_same_nodes():
    """The half-covered graph of test_gpu_graph.py::test_frame_loop_inserts_nodes_where_the_graph_has_none at R = 64."""
    K, scale, center, tdist, lws, depth = _scene()
    node_pos, node_w = scene.fibonacci_nodes(256, R)
    front = node_pos[:, 0] < R / 2
    first = [depth(lw) for lw in lws]
    graphs = {}
    for sampler in ("host", "device"):
        sf = _frame(K, scale, center, tdist, node_pos[front], node_w[front])
        for d, lw in zip(first, lws):
            sf.integrate(d, lw)
        sf.refresh_samples()
        sv = sf.fs.solver
        n0 = sv.N
        assert int(graph.unsupported_vertices(sv.spos, sv.snbr, sv.node_pos, sv.node_w).sum()) > 100
        n_new = sf.update_graph(sampler=sampler)
        assert n_new > 5 and sv.N == n0 + n_new
        assert int(graph.unsupported_vertices(sv.spos, sv.snbr, sv.node_pos, sv.node_w).sum()) == 0
        graphs[sampler] = (sv.node_pos.clone(), sv.node_dq.clone(), sv.node_w.clone())
    for a, b in zip(graphs["host"], graphs["device"]):
        assert torch.equal(a, b)
    # and through step(update_graph=True, graph_sampler="device"): nothing left to insert, the loop runs
    n = sf.step(first, lws, gn_iters=2, update_graph=True, graph_sampler="device")
    assert n == sv.S and 0 <= sv.N - graphs["device"][0].shape[0] <= 3  # (a moving band may still expose a point)
