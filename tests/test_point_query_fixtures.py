"""CPU: the inputs of tests/test_gpu_point_queries.py (tests/point_query_cases.py) are what they claim to be -- proved with the numpy
oracle alone, where there is no GPU: the exact ties, the ratios of exactly 1, the costs of exactly the tolerance, the rows whose
every neighbour costs 1 or more, the blends that vanish to exactly 0, the positions that are no float32 numbers, the non-finite
rows -- and the new restatements in oracle/oracle_np.py agree with independent formulations."""
import numpy as np
import pytest

import point_query_cases as C
from oracle import gn_np as G
from oracle import oracle_np as O


def _d2(a, b):
    d = a[:, None, :] - b[None, :, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


# ------------------------------------------------------------------------------------------------ dfh_closest_correspondences
@pytest.mark.parametrize("knn", C.KNNS)
def test_closest_cases_hold_their_boundaries(knn):
    seen = set()
    for n_live in C.closest_live_sizes(knn):
        for n_verts in C.CLOSEST_VERTS:
            c = C.closest_case(knn, n_live, n_verts)
            pos, nrm, live, rows = c["pos"], c["nrm"], c["live"], c["rows"]
            assert pos.shape == nrm.shape == (n_verts, 3) and live.shape == (n_live, 3)
            assert np.isfinite(pos).all() and pos.min() >= -5 and pos.max() <= 60 and live.min() >= -5 and live.max() <= 60
            nidx = O.knn_bruteforce(pos, live, knn)
            d = pos[:, None, :] - live[nidx]
            with np.errstate(invalid="ignore"):
                cost = np.abs(nrm[:, None, 0] * d[..., 0] + nrm[:, None, 1] * d[..., 1] + nrm[:, None, 2] * d[..., 2])
            best, best_cost, _ = O.closest_correspondences(pos, nrm, live, knn, 0.2)
            d2 = _d2(pos, live)
            for a, b in c["dups"]:
                assert a < b and np.array_equal(live[a], live[b])
            if n_live >= 257:
                assert (255, 256) in c["dups"]                                    # duplicates across the tile boundary
            for r in rows.get("tile_tie", []):
                lo, hi = c["tile_pair"]
                assert lo < hi and not np.array_equal(live[lo], live[hi])
                assert d2[r, lo] == d2[r, hi] == d2[r].min() and (d2[r] == d2[r].min()).sum() == 2       # an exact distance tie ...
                assert nidx[r, 0] == lo and (knn == 1 or nidx[r, 1] == hi)
                if knn >= 2:
                    assert cost[r, 0] == cost[r, 1] == cost[r].min() == 0.125     # ... and an exact cost tie: the first one wins
                assert np.array_equal(best[r], live[lo])
                if n_live >= 258:
                    assert lo < C.TILE <= hi
            for r in rows["all_ge_1"]:
                assert (cost[r] >= 1.0).all() and best_cost[r] == 1.0 and np.array_equal(best[r], live[nidx[r, 0]])
            for r in rows.get("cost_1", []):
                assert cost[r, 0] == 1.0
            for r in rows.get("cost_eq_tol", []):
                assert best_cost[r] in C.TOLERANCES and best_cost[r] < 1.0
            for r, e in zip(rows.get("cost_above_tol", []), rows.get("cost_eq_tol", [])):
                assert best_cost[r] == np.nextafter(best_cost[e], 1.0)
            for r in rows["nan_normal"]:
                assert np.isnan(cost[r]).all() and best_cost[r] == 1.0 and np.array_equal(best[r], live[nidx[r, 0]])
            # natural ties between DIFFERENT live points at the boundary of the k nearest (the stable order decides who is in)
            if n_live > knn:
                srt = np.sort(d2, axis=1)
                if (srt[:, knn - 1] == srt[:, knn]).any():
                    seen.add("kth_tie")
            if knn >= 2 and ((cost[:, :, None] == cost[:, None, :]) & ~np.eye(knn, dtype=bool) & (cost[:, :, None] < 1)).any():
                seen.add("cost_tie")
            if n_live >= 255 and n_verts >= 255:
                assert {"tile_tie", "all_ge_1", "cost_1", "cost_eq_tol", "cost_above_tol", "nan_normal", "dup"} <= {k for k, v in rows.items() if v}
                assert 0 < (best_cost < 1).sum() < n_verts and (best_cost <= 0.2).any()
            seen |= {k for k, v in rows.items() if v}
    assert {"kth_tie", "tile_tie", "cost_eq_tol", "dup"} <= seen and (knn == 1 or "cost_tie" in seen)


def test_closest_nonfinite_rows_and_the_oracle_contract():
    c = C.closest_case(4, 257, 257, nonfinite=True)
    bad = c["rows"]["nonfinite"]
    assert len(bad) == 4 and not np.isfinite(c["pos"][bad]).all(axis=1).any()
    assert np.isnan(c["pos"][bad]).any() and np.isposinf(c["pos"][bad]).any() and np.isneginf(c["pos"][bad]).any()
    best, cost, keep = O.closest_correspondences(c["pos"], c["nrm"], c["live"], 4, 1.0)
    assert np.array_equal(best[bad], np.zeros((4, 3))) and np.isposinf(cost[bad]).all() and not keep[bad].any()
    ok = np.setdiff1d(np.arange(257), bad)
    assert np.isfinite(best[ok]).all() and (cost[ok] <= 1.0).all() and keep[ok].all()


# ------------------------------------------------------------------------------------------------ dfh_nearest_points
def test_nearest_cases_hold_their_ties():
    kinds = set()
    for n_cloud in C.NEAREST_CLOUDS:
        for n_query in C.NEAREST_QUERIES:
            c = C.nearest_case(n_cloud, n_query)
            cloud, query = c["cloud"], c["query"]
            assert cloud.shape == (n_cloud, 3) and query.shape == (n_query, 3)
            idx, d2 = O.nearest_points(query, cloud)
            full = _d2(query, cloud)
            assert np.array_equal(idx, full.argmin(axis=1)) and np.array_equal(d2, full.min(axis=1))
            for q, (lo, hi) in c["ties"].items():
                assert lo < hi and full[q, lo] == full[q, hi] == full[q].min() and idx[q] == lo
                t_lo, t_hi = lo % C.TILE, hi % C.TILE                        # the threads that hold the two points
                kinds.add("cross" if t_lo > t_hi else "same" if t_lo == t_hi else "next" if t_hi == t_lo + 1 else "apart")
            if n_cloud >= 12:
                assert len(c["ties"]) == min(3 if n_cloud == 1000 else 2, n_query)
            if n_query == 300:
                assert (d2 == 0).sum() >= 4
    assert {"cross", "same", "next"} <= kinds
    c = C.nearest_case(1000, 300, nonfinite=True)
    idx, d2 = O.nearest_points(c["query"], c["cloud"])
    bad = c["nonfinite"]
    assert len(bad) == 3 and (idx[bad] == -1).all() and np.isposinf(d2[bad]).all() and (np.delete(idx, bad) >= 0).all()


# ------------------------------------------------------------------------------------------------ dfh_graph_unsupported
@pytest.mark.parametrize("knn", C.KNNS)
def test_unsupported_cases_sit_on_the_ratio_of_one(knn):
    for n_verts in C.GRAPH_VERTS:
        c = C.unsupported_case(knn, n_verts)
        v, nbr, npos, nw, rows = c["verts"], c["nbr"], c["node_pos"], c["node_w"], c["rows"]
        assert nbr.shape == (n_verts, knn) and nbr.min() >= 0 and nbr.max() < len(npos)
        d = npos[nbr] - v[:, None, :]
        ratio = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) / nw[nbr]
        flag = O.unsupported_vertices(v, nbr, npos, nw)
        assert np.array_equal(flag, ratio.min(axis=1) >= 1)
        assert len(rows["at_1"]) == len(rows["inside"]) == len(rows["inside_w"]) == knn
        for slot, r in enumerate(rows["at_1"]):
            assert ratio[r].min() == 1.0 == ratio[r, slot] and (np.delete(ratio[r], slot) > 1).all() and flag[r]
        for name in ("inside", "inside_w"):
            for slot, r in enumerate(rows[name]):
                assert 1.0 - 1e-15 < ratio[r, slot] < 1.0 and (np.delete(ratio[r], slot) > 1).all() and not flag[r]
        assert 0 < flag.sum() < n_verts


# ------------------------------------------------------------------------------------------------ the warp family
@pytest.mark.parametrize("knn", C.KNNS)
def test_blend_cases_vanish_exactly(knn):
    c = C.blend_case(knn)
    pts, nbr, npos, nw, ndq, rows = c["pts"], c["nbr"], c["node_pos"], c["node_w"], c["node_dq"], c["rows"]
    w = G.blend_weights(pts, npos[nbr], nw[nbr])
    raw = (w[..., None] * ndq[nbr]).sum(axis=1)
    out = O.dq_blend(pts, ndq[nbr], npos[nbr], nw[nbr])
    ident = np.eye(8)[0]
    assert rows["underflow"] and (knn == 1 or rows["cancel"])
    for r in rows["underflow"]:
        assert (w[r] == 0).all() and np.array_equal(out[r], ident)
    for r in rows["cancel"]:
        assert (w[r] > 0).sum() == knn - knn % 2 and w[r].max() > 0.1 and np.array_equal(raw[r], np.zeros(8)) and np.array_equal(out[r], ident)
        acc = np.zeros(8)
        for j in range(knn):                                                # in the kernel's order too: exactly 0 after every pair
            acc = acc + w[r, j] * ndq[nbr[r, j]]
        assert np.array_equal(acc, np.zeros(8))
    rest = np.setdiff1d(np.arange(len(pts)), rows["underflow"] + rows["cancel"])
    assert np.abs(np.linalg.norm(out[rest], axis=1) - 1).max() < 1e-14 and (np.abs(raw[rest]).max(axis=1) > 0).all()
    assert np.abs(np.linalg.norm(ndq[:, :4], axis=1) - 1).max() < 1e-15 and np.abs((ndq[:, :4] * ndq[:, 4:]).sum(axis=1)).max() < 1e-15


def test_warp_cases_are_no_float32_numbers():
    for knn in (1, 8):
        for n_verts in C.GRAPH_VERTS:
            c = C.warp_case(knn, n_verts)
            for name in ("verts", "nrm", "node_pos"):
                a = c[name]
                err = np.abs(a.astype(np.float32).astype(np.float64) - a)
                assert (err > 0).all(), name                                 # every single coordinate changes when rounded
            assert c["nbr"].shape == (n_verts, knn) and c["node_nbr"].shape == (n_verts, knn) and len(c["node_pos"]) == n_verts
            # a warp that skips the rounding of the position moves the result by far more than the 1e-12 bar
            pw = O.warp(c["verts"], c["node_dq"][c["nbr"]], c["node_pos"][c["nbr"]], c["node_w"][c["nbr"]], m_lw=c["lw"])
            v32 = c["verts"].astype(np.float32).astype(np.float64)
            assert np.abs(pw - O.warp(v32, c["node_dq"][c["nbr"]], c["node_pos"][c["nbr"]], c["node_w"][c["nbr"]], m_lw=c["lw"])).max() < 1e-5
            assert np.abs(c["verts"] - v32).max() > 1e-7
            assert np.isfinite(pw).all() and np.linalg.norm(pw - c["verts"], axis=1).min() > 0.01                    # a real warp


def test_sample_knn_case_and_oracle():
    c = C.sample_knn_case(700, 4)
    bad = c["nonfinite"]
    assert not np.isfinite(c["pts"][bad]).all(axis=1).any() and np.isfinite(np.delete(c["pts"], bad, axis=0)).all()
    assert min(bad) < C.TILE <= max(bad) and max(bad) < 2 * C.TILE < len(c["pts"])     # two workgroups hit, the third clean
    nbr, w = O.sample_knn(c["pts"], c["node_pos"], c["node_w"], 4)
    nbr_f, w_f = O.sample_knn(c["finite"], c["node_pos"], c["node_w"], 4)
    ok = np.setdiff1d(np.arange(len(nbr)), bad)
    assert np.array_equal(nbr[bad], np.tile(np.arange(4), (4, 1))) and (w[bad] == 0).all()
    assert np.array_equal(nbr[ok], nbr_f[ok]) and np.array_equal(w[ok], w_f[ok])
    assert np.array_equal(nbr_f, O.knn_bruteforce(c["finite"], c["node_pos"], 4))
    assert np.abs(w_f - G.blend_weights(c["finite"], c["node_pos"][nbr_f], c["node_w"][nbr_f])).max() <= 4e-16


# ------------------------------------------------------------------------------------------------ permute, pack, unpack
def test_permute_and_pack_oracles():
    rng = np.random.default_rng(5)
    S, k = 257, 3
    order = rng.permutation(S)
    arrs = (rng.normal(size=(S, 3)), rng.normal(size=(S, 3)), rng.integers(0, 9, size=(S, k)).astype(np.int32), rng.normal(size=(S, k)))
    out = O.permute_samples(order, *arrs)
    for a, o in zip(arrs, out):
        assert all(np.array_equal(o[i], a[order[i]]) for i in range(S))
    # a symmetric pattern: the diagonal and a few pairs, sorted by (row, col) like the solver's
    N = 7
    pairs = {(i, i) for i in range(N)} | {(0, 3), (3, 0), (2, 5), (5, 2), (1, 6), (6, 1), (4, 5), (5, 4)}
    keys = np.array(sorted(r * N + c for r, c in pairs))
    rows, col = keys // N, keys % N
    upper = col >= rows
    rank = np.cumsum(upper) - 1
    mirror = np.searchsorted(keys, col * N + rows)
    src = np.where(upper, rank, rank[mirror])
    n_upper = int(upper.sum())
    sym = C.block_system(rng, rows, col, N, symmetric=True)
    packed = O.pack_upper(sym, rows, col, src, N, n_upper)
    assert packed.shape == (36 * n_upper + 6 * N + 2,) and n_upper == N + 4
    assert np.array_equal(O.unpack_upper(packed, rows, col, src, N, n_upper), sym)
    assert np.array_equal(packed[36 * n_upper:], sym[36 * len(col):])
    for b in np.nonzero(upper)[0]:
        assert np.array_equal(packed[36 * src[b]:36 * src[b] + 36], sym[36 * b:36 * b + 36])
    raw = C.block_system(rng, rows, col, N, symmetric=False)
    back = O.unpack_upper(O.pack_upper(raw, rows, col, src, N, n_upper), rows, col, src, N, n_upper)
    B = len(col)
    for b in range(B):
        blk = back[36 * b:36 * b + 36].reshape(6, 6)
        if upper[b]:
            assert np.array_equal(blk, raw[36 * b:36 * b + 36].reshape(6, 6))
        else:
            m = mirror[b]
            assert np.array_equal(blk, raw[36 * m:36 * m + 36].reshape(6, 6).T) and not np.array_equal(blk, raw[36 * b:36 * b + 36].reshape(6, 6))
    assert np.array_equal(back[36 * B:], raw[36 * B:])
