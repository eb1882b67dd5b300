"""GPU: the small kernels that feed the solver and maintain the deformation graph against fp64 restatements of their definitions
(oracle/oracle_np.py), at every knn, at the edges of the 256-row workgroup / LDS tile and on exact ties -- inputs from
tests/point_query_cases.py, which tests/test_point_query_fixtures.py proves to sit on the boundaries they claim.

Bars.  Indices, flags, `keep`, the chosen live row (`corr`) and the squared distance of dfh_nearest_points are EXACT: the oracle
performs the same fp64 operations in the same order ((a + b) + c, the build switches contraction off) and resolves ties by stable
order like the kernels.  Whatever passes through the device's exp or a longer chain -- costs, blends, warps, residuals -- is held to
1e-12 absolute, the bar of the golden tests of the same kernels (test_gpu_solve.py, test_gpu_graph.py: device exp against libm).
dfh_permute_samples and the pack / unpack pair move bits: exact.  No row of any case is excluded from a comparison."""
import numpy as np
import pytest
import torch

import point_query_cases as C
from dynamicfusion_body_amd import _lib, graph, kernels, solve
from dynamicfusion_body_amd.device import current_stream_ptr
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

BAR = 1e-12
IDENT = np.eye(8)[0]


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def closest(P, Nn, Lv, knn, tol, with_cost=True):
    """dfh_closest_correspondences through ctypes (cost_out may be NULL) on device tensors -> numpy (corr, cost or None, keep)."""
    V = P.shape[0]
    corr = torch.full((V, 3), -7.0, dtype=torch.float64, device="cuda")
    cost = torch.full((V,), -7.0, dtype=torch.float64, device="cuda")
    keep = torch.full((V,), 7, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.load().dfh_closest_correspondences(P.data_ptr(), Nn.data_ptr(), V, Lv.data_ptr(), Lv.shape[0], knn, float(tol), corr.data_ptr(),
                                                       cost.data_ptr() if with_cost else None, keep.data_ptr(), current_stream_ptr()),
               "dfh_closest_correspondences")
    return corr.cpu().numpy(), cost.cpu().numpy() if with_cost else None, keep.cpu().numpy()


def check_closest(c, knn):
    P, Nn, Lv = dev(c["pos"]), dev(c["nrm"]), dev(c["live"])
    best, best_cost, _ = O.closest_correspondences(c["pos"], c["nrm"], c["live"], knn, 0.0)
    for tol in C.TOLERANCES:
        corr, cost, keep = closest(P, Nn, Lv, knn, tol)
        assert np.array_equal(corr, best), (knn, len(c["live"]), len(c["pos"]), np.nonzero((corr != best).any(axis=1))[0][:8])
        with np.errstate(invalid="ignore"):
            err = np.where(cost == best_cost, 0.0, np.abs(cost - best_cost))          # (inf == inf on the rows without neighbours)
        assert err.max() <= BAR
        assert np.array_equal(keep, (best_cost <= tol).astype(np.uint8)), (knn, tol)
    return P, Nn, Lv, best, best_cost


@pytest.mark.parametrize("knn", C.KNNS)
def test_closest_correspondences_vs_oracle(knn):
    """Every n_live in {knn, 255, 256, 257, 513} x n_verts in {1, 255, 256, 257} x tolerance in {0.2, 0.25, 1}: duplicated live
    vertices (one pair across the tile boundary), two different live points at the same distance and cost on either side of it (the
    lower index wins), rows whose every cost is >= 1 (best = nearest, cost = 1, kept iff 1 <= tolerance), a cost of exactly the
    tolerance (kept) and one double above (not kept), a NaN normal at a finite position."""
    for n_live in C.closest_live_sizes(knn):
        for n_verts in C.CLOSEST_VERTS:
            c = C.closest_case(knn, n_live, n_verts)
            P, Nn, Lv, best, best_cost = check_closest(c, knn)
            rows = c["rows"]
            if n_verts >= 255 and n_live >= 255:                              # the crafted rows, spelled out (the oracle agrees: CPU test)
                corr, cost, keep = closest(P, Nn, Lv, knn, 0.2)
                assert np.array_equal(corr[rows["tile_tie"][0]], c["live"][c["tile_pair"][0]])
                assert (cost[rows["all_ge_1"]] == 1.0).all() and not keep[rows["all_ge_1"]].any()
                assert cost[rows["cost_eq_tol"][0]] == 0.2 and keep[rows["cost_eq_tol"][0]] == 1 and keep[rows["cost_above_tol"][0]] == 0
                assert cost[rows["nan_normal"][0]] == 1.0
                keep1 = closest(P, Nn, Lv, knn, 1.0)[2]
                assert keep1[rows["all_ge_1"]].all() and keep1[rows["nan_normal"]].all()
    corr, cost, keep = closest(P, Nn, Lv, knn, 0.25, with_cost=False)           # cost_out = NULL (the last, largest case)
    assert cost is None and np.array_equal(corr, best) and np.array_equal(keep, (best_cost <= 0.25).astype(np.uint8))
    assert np.array_equal(solve.closest_correspondences(P, Nn, Lv, knn, 0.25)[0].cpu().numpy(), best)       # the Python wrapper


def nearest(Q, Cl, with_d2):
    idx = torch.full((Q.shape[0],), -9, dtype=torch.int32, device="cuda")
    d2 = torch.full((Q.shape[0],), -9.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().dfh_nearest_points(Q.data_ptr(), Q.shape[0], Cl.data_ptr(), Cl.shape[0], idx.data_ptr(),
                                              d2.data_ptr() if with_d2 else None, current_stream_ptr()), "dfh_nearest_points")
    return idx.cpu().numpy(), d2.cpu().numpy()


def test_nearest_points_vs_oracle():
    """n_cloud in {1, 255, 256, 257, 1000} x n_query in {1, 3, 300}, d2_out given and NULL: idx exact, d2 bit-equal; exact ties
    inside one thread's scan (j, j + 256), between neighbouring threads, and with the lower index in the higher thread (5, 258)."""
    for n_cloud in C.NEAREST_CLOUDS:
        for n_query in C.NEAREST_QUERIES:
            c = C.nearest_case(n_cloud, n_query)
            Q, Cl = dev(c["query"]), dev(c["cloud"])
            want_idx, want_d2 = O.nearest_points(c["query"], c["cloud"])
            idx, d2 = nearest(Q, Cl, True)
            assert np.array_equal(idx, want_idx), (n_cloud, n_query, np.nonzero(idx != want_idx)[0][:8], c["ties"])
            assert np.array_equal(d2, want_d2), (n_cloud, n_query, np.abs(d2 - want_d2).max())
            for q, (lo, hi) in c["ties"].items():
                assert idx[q] == lo
            idx0, d20 = nearest(Q, Cl, False)
            assert np.array_equal(idx0, want_idx) and (d20 == -9.0).all()      # NULL: nothing written anywhere
            assert np.array_equal(graph.nearest_points(Q, Cl).cpu().numpy(), want_idx)


@pytest.mark.parametrize("knn", C.KNNS)
def test_graph_unsupported_vs_oracle(knn):
    """Vertices at exactly the node's weight from their nearest listed node (offset (3, 4, 0), w = 5: ratio exactly 1) are flagged,
    vertices one ulp inside are not; the deciding node at every position of the list."""
    for n_verts in C.GRAPH_VERTS:
        c = C.unsupported_case(knn, n_verts)
        flag = graph.unsupported_vertices(c["verts"], dev(c["nbr"], torch.int32), c["node_pos"], c["node_w"]).cpu().numpy()
        want = O.unsupported_vertices(c["verts"], c["nbr"], c["node_pos"], c["node_w"])
        assert np.array_equal(flag, want.astype(np.uint8)), (knn, n_verts, np.nonzero(flag != want)[0][:8])
        assert flag[c["rows"]["at_1"]].all() and not flag[c["rows"]["inside"]].any() and not flag[c["rows"]["inside_w"]].any()


@pytest.mark.parametrize("knn", C.KNNS)
def test_dq_blend_points_vs_oracle(knn):
    """Against Fusion.dq_blend's restatement; every weight underflowing to 0 and a pair q, -q at equal distance both give a blend
    of exactly 0: the identity, exactly."""
    c = C.blend_case(knn)
    nbr = c["nbr"]
    out = graph.dq_blend_points(c["pts"], dev(nbr, torch.int32), c["node_dq"], c["node_pos"], c["node_w"]).cpu().numpy()
    want = O.dq_blend(c["pts"], c["node_dq"][nbr], c["node_pos"][nbr], c["node_w"][nbr])
    err = np.abs(out - want).max(axis=1)
    assert err.max() <= BAR, (knn, int(err.argmax()), err.max())
    for r in c["rows"]["underflow"] + c["rows"]["cancel"]:
        assert np.array_equal(out[r], IDENT), (knn, r, out[r])


def warp(c, nbr=True, normals=True, out_nrm=True):
    """dfh_warp_points through ctypes, so that normals can be given without out_nrm."""
    V = dev(c["verts"])
    Nn = dev(c["nrm"]) if normals else None
    op = torch.full_like(V, -7.0)
    on = torch.full_like(V, -7.0)
    if nbr:
        nb, Q, P, Wn = dev(c["nbr"], torch.int32), dev(c["node_dq"]), dev(c["node_pos"]), dev(c["node_w"])
        args = (nb.data_ptr(), V.shape[0], c["knn"], Q.data_ptr(), P.data_ptr(), Wn.data_ptr(), Q.shape[0])
    else:
        args = (None, V.shape[0], c["knn"], None, None, None, 0)
    _lib.check(_lib.load().dfh_warp_points(V.data_ptr(), Nn.data_ptr() if normals else None, *args, _lib.darr(c["lw"], 8), op.data_ptr(),
                                           on.data_ptr() if out_nrm else None, current_stream_ptr()), "dfh_warp_points")
    return op.cpu().numpy(), on.cpu().numpy()


@pytest.mark.parametrize("knn", C.KNNS)
def test_warp_points_vs_oracle(knn):
    """Against Fusion.warp's restatement at n_verts in {255, 256, 257}: with and without the graph (nbr = NULL), with and without
    normals, and normals given with out_nrm = NULL.  No input is a float32 number: a dropped round to float32 is ~1e-6."""
    for n_verts in C.GRAPH_VERTS:
        c = C.warp_case(knn, n_verts)
        nbr = c["nbr"]
        wp, wn = O.warp(c["verts"], c["node_dq"][nbr], c["node_pos"][nbr], c["node_w"][nbr], normal=c["nrm"], m_lw=c["lw"])
        p, n = warp(c)
        assert np.abs(p - wp).max() <= BAR and np.abs(n - wn).max() <= BAR, (knn, n_verts, np.abs(p - wp).max(), np.abs(n - wn).max())
        p1, n1 = warp(c, out_nrm=False)                                     # normals without out_nrm: positions only
        assert np.array_equal(p1, p) and (n1 == -7.0).all()
        p2, n2 = warp(c, normals=False, out_nrm=False)
        assert np.array_equal(p2, p) and (n2 == -7.0).all()
        p3, n3 = warp(c, nbr=False)                                         # the global transform alone (FusionDM)
        assert np.abs(p3 - O.dqb_warp(c["lw"], c["verts"])).max() <= BAR and np.abs(n3 - O.dqb_warp_normal(c["lw"], c["nrm"])).max() <= BAR
        p4, n4 = warp(c, nbr=False, normals=False, out_nrm=False)
        assert np.array_equal(p4, p3) and (n4 == -7.0).all()
        # and the Python wrapper's three forms
        q, m = solve.warp_points(c["verts"], c["nrm"], c["lw"], nbr, c["node_dq"], c["node_pos"], c["node_w"])
        assert np.array_equal(q.cpu().numpy(), p) and np.array_equal(m.cpu().numpy(), n)
        q, m = solve.warp_points(c["verts"], None, c["lw"], nbr, c["node_dq"], c["node_pos"], c["node_w"])
        assert np.array_equal(q.cpu().numpy(), p) and m is None
        q, m = solve.warp_points(c["verts"], c["nrm"], c["lw"])
        assert np.array_equal(q.cpu().numpy(), p3) and np.array_equal(m.cpu().numpy(), n3)


@pytest.mark.parametrize("knn", C.KNNS)
def test_residuals_vs_oracle(knn):
    """dfh_residual_data against computef_data and dfh_residual_reg against computef_reg at 255, 256 and 257 vertices / nodes."""
    for n in C.GRAPH_VERTS:
        c = C.warp_case(knn, n)
        fd = solve.residual_data(c["node_dq"], c["verts"], c["nrm"], c["corr"], c["nbr"], c["node_pos"], c["node_w"], c["lw"]).cpu().numpy()
        want = O.computef_data(c["node_dq"], c["verts"], c["nrm"], c["corr"], c["nbr"], c["node_pos"], c["node_w"], c["lw"])
        assert fd.shape == want.shape and np.abs(fd - want).max() <= BAR, (knn, n, np.abs(fd - want).max())
        rw = 0.375
        fr = solve.residual_reg(c["node_dq"], c["node_nbr"], c["node_pos"], c["node_w"], rw).cpu().numpy()
        want = O.computef_reg(c["node_dq"], np.arange(n), c["node_nbr"], c["node_pos"], c["node_w"], rw)
        assert fr.shape == want.shape == (3 * n * knn,) and np.abs(fr - want).max() <= BAR, (knn, n, np.abs(fr - want).max())
        assert np.abs(want).max() > 1e-3


def test_permute_samples_is_fancy_indexing():
    lib = _lib.load()
    rng = np.random.default_rng(11)
    for knn in (1, 3, 8):
        for S in (1, 257):
            order = rng.permutation(S)
            arrs = (rng.normal(size=(S, 3)), rng.normal(size=(S, 3)), rng.integers(0, 1 << 30, size=(S, knn)).astype(np.int32),
                    rng.normal(size=(S, knn)))
            d = [dev(a, torch.int32 if a.dtype == np.int32 else torch.float64) for a in arrs]
            out = [torch.full_like(t, -7) for t in d]
            od = dev(order, torch.int64)
            _lib.check(lib.dfh_permute_samples(od.data_ptr(), S, knn, *[t.data_ptr() for t in d], *[t.data_ptr() for t in out],
                                               current_stream_ptr()), "dfh_permute_samples")
            for got, want in zip(out, O.permute_samples(order, *arrs)):
                assert np.array_equal(got.cpu().numpy(), want), (knn, S)


@pytest.mark.parametrize("N", [1, 40])
def test_pack_and_unpack_upper_single_process(N):
    """dfh_gn_pack_upper / dfh_gn_unpack_upper without a collective, on the pattern and the rows / src / n_upper tables that
    WarpSolver._build_pattern itself builds for the sharded solve: a symmetric system survives pack -> unpack bit for bit and
    `packed` is the oracle's; on a system whose lower blocks are NOT the transposes, unpack writes the transposed upper blocks
    into the lower positions and leaves the tail (J^T r, cost, count) exact."""
    lib = _lib.load()
    rng = np.random.default_rng(N)
    k = min(4, N)
    npos = rng.uniform(5.0, 45.0, size=(N, 3))
    _lib.set_option("py_plan_torch", 1)                                     # (the plan is not under test: the host-side builder)
    sv = solve.WarpSolver(knn=k, pcg_iters=4, distributed=True)
    sv.force_collective = True                                              # the tables of the sharded solve in a group of one
    sv.set_graph(npos, C.unit_dqs(rng, N), rng.uniform(3.0, 6.0, size=N), node_nbr=O.knn_bruteforce(npos, npos, k))
    pts = rng.uniform(5.0, 45.0, size=(60, 3))
    sv.set_samples(pts, pts * 0 + [0.0, 0.0, 1.0])
    sv.prepare()
    assert sv._tri is not None
    rows_d, src_d, n_upper, packed_d = sv._tri
    rows, col, src = rows_d.cpu().numpy(), sv.col.cpu().numpy(), src_d.cpu().numpy()
    B = sv.B
    assert B == len(col) == len(rows) == len(src) and n_upper == int((col >= rows).sum()) and (B == 1 if N == 1 else B > N + 10)
    assert sv.system.numel() == 36 * B + 6 * N + 2 and packed_d.numel() == 36 * n_upper + 6 * N + 2

    def pack(system):
        sysd, pk = dev(system), torch.full_like(packed_d, -7.0)
        _lib.check(lib.dfh_gn_pack_upper(sysd.data_ptr(), rows_d.data_ptr(), sv.col.data_ptr(), src_d.data_ptr(), B, N, n_upper, pk.data_ptr(),
                                         current_stream_ptr()), "dfh_gn_pack_upper")
        return pk

    def unpack(pk):
        sysd = torch.full((36 * B + 6 * N + 2,), -7.0, dtype=torch.float64, device="cuda")
        _lib.check(lib.dfh_gn_unpack_upper(sysd.data_ptr(), rows_d.data_ptr(), sv.col.data_ptr(), src_d.data_ptr(), B, N, n_upper, pk.data_ptr(),
                                           current_stream_ptr()), "dfh_gn_unpack_upper")
        return sysd.cpu().numpy()

    sym = C.block_system(rng, rows, col, N, symmetric=True)
    pk = pack(sym)
    assert np.array_equal(pk.cpu().numpy(), O.pack_upper(sym, rows, col, src, N, n_upper))
    assert np.array_equal(unpack(pk), sym)
    raw = C.block_system(rng, rows, col, N, symmetric=False)
    pk = pack(raw)
    assert np.array_equal(pk.cpu().numpy(), O.pack_upper(raw, rows, col, src, N, n_upper))
    back = unpack(pk)
    want = O.unpack_upper(pk.cpu().numpy(), rows, col, src, N, n_upper)
    assert np.array_equal(back, want)
    assert np.array_equal(back[36 * B:], raw[36 * B:])                      # the tail
    up = col >= rows
    rb, bb = raw[:36 * B].reshape(B, 6, 6), back[:36 * B].reshape(B, 6, 6)
    assert np.array_equal(bb[up], rb[up])
    if N > 1:
        where = {(int(r), int(c_)): b for b, (r, c_) in enumerate(zip(rows, col))}
        lower = np.nonzero(~up)[0]
        assert len(lower) == B - n_upper > 5
        for b in lower:
            assert np.array_equal(bb[b], rb[where[(int(col[b]), int(rows[b]))]].T) and not np.array_equal(bb[b], rb[b])


# ------------------------------------------------------------------------------------------------ non-finite rows
# (include/dfusion_hip.h defines them; before that definition such a row read live[3 * (-1)] and node_w[-1])
def test_closest_correspondences_nonfinite_positions():
    """corr = (0, 0, 0), cost = +inf, keep = 0 whatever the tolerance; every other row as the oracle has it."""
    for knn, n_live in ((1, 1), (4, 257), (8, 513)):
        c = C.closest_case(knn, n_live, 257, nonfinite=True)
        P, Nn, Lv, best, best_cost = check_closest(c, knn)
        bad = c["rows"]["nonfinite"]
        for tol in (1.0, np.inf):
            corr, cost, keep = closest(P, Nn, Lv, knn, tol)
            assert np.array_equal(corr[bad], np.zeros((len(bad), 3))) and np.isposinf(cost[bad]).all() and not keep[bad].any()
            assert np.array_equal(corr, best) and np.array_equal(keep, (best_cost <= 1.0).astype(np.uint8))
        assert np.array_equal(closest(P, Nn, Lv, knn, 1.0, with_cost=False)[0], best)


def test_nearest_points_nonfinite_queries():
    c = C.nearest_case(1000, 300, nonfinite=True)
    want_idx, want_d2 = O.nearest_points(c["query"], c["cloud"])
    for with_d2 in (True, False):
        idx, d2 = nearest(dev(c["query"]), dev(c["cloud"]), with_d2)
        assert np.array_equal(idx, want_idx) and (idx[c["nonfinite"]] == -1).all()
        if with_d2:
            assert np.array_equal(d2, want_d2) and np.isposinf(d2[c["nonfinite"]]).all()


@pytest.mark.parametrize("n_nodes,knn", [(700, 4), (300, 8), (9, 8), (40, 1)])
def test_sample_knn_nonfinite_samples(n_nodes, knn):
    """nbr = 0..knn-1 and weights 0 for a non-finite sample, through the bounding-box pruning (300 nodes), the plain scan (700 nodes:
    more candidates than fit) and the brick lists; the finite samples of the same workgroups keep their bits (against a run
    in which the non-finite rows are ordinary points); dfh_sample_knn_bricks == dfh_sample_knn bit for bit."""
    c = C.sample_knn_case(n_nodes, knn)
    bad = c["nonfinite"]
    ok = np.setdiff1d(np.arange(len(c["pts"])), bad)
    nbr, w = solve.sample_knn(c["pts"], c["node_pos"], c["node_w"], knn)
    nbr_f, w_f = solve.sample_knn(c["finite"], c["node_pos"], c["node_w"], knn)
    want_nbr, want_w = O.sample_knn(c["pts"], c["node_pos"], c["node_w"], knn)
    n_, w_ = nbr.cpu().numpy(), w.cpu().numpy()
    assert np.array_equal(n_, want_nbr) and np.abs(w_ - want_w).max() <= 4e-15
    assert np.array_equal(n_[bad], np.tile(np.arange(knn), (len(bad), 1))) and (w_[bad] == 0).all()
    assert np.array_equal(n_[ok], nbr_f.cpu().numpy()[ok]) and np.array_equal(w_[ok], w_f.cpu().numpy()[ok])
    res, slab = (32, 40, 48), (4, 30)
    ws = kernels.dqb_workspace(res, slab, knn=knn, n_nodes=n_nodes)
    kernels.dqb_build_candidates(ws, res, c["node_pos"], knn, slab)
    nbr_b, w_b = solve.sample_knn(c["pts"], c["node_pos"], c["node_w"], knn, bricks=(res, slab, ws))
    assert torch.equal(nbr_b, nbr) and torch.equal(w_b, w)
    inside = np.all((np.rint(c["finite"]) >= [slab[0], 0, 0]) & (np.rint(c["finite"]) <= [slab[1] - 1, res[1] - 1, res[2] - 1]), axis=1)
    assert inside.any() and (~inside).any()                                 # the lists and the full scan were both used
