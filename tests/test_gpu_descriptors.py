"""GPU: dfh_nearest_descriptors (K14) against the numpy restatement of its definition (tests/descriptors_np.py): the indices are
np.array_equal and the squared distances bit-equal, on the exact kernel (nd_path = 1) and on the fast path (nd_path = 2) alike;
then the CNN branch of Fusion.setupCorrespondences against a numpy restatement of the reference's core/fusion.py:277-313, and
what descriptor correspondences buy the `_lw` pre-fit on a body that turns about its own axis."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import descriptors_np as DN
from oracle import gn_np as G
from oracle import oracle_np as O
from dynamicfusion_body_amd import Fusion, _lib, solve
from dynamicfusion_body_amd.device import current_stream_ptr

pytestmark = pytest.mark.gpu

PATHS = [1, 2]
# the kernels as built (dfh_nearest_descriptors_tile): the score kernel's workgroup takes TILE_Q queries (four waves of 32) and
# walks the base in LDS chunks of TILE_B rows (four 32 x 32 matrix-core tiles each); the exact kernel takes EXACT_Q queries per
# workgroup and stages 4096 // dim base rows at a time; a query has SLOTS candidate slots
MFMA, TILE_Q, TILE_B, EXACT_Q, SLOTS, EXACT_FLOATS = 32, 128, 128, 256, 32, 4096
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "descriptor_recovery.json")


def test_tile_constants_are_the_kernels():
    tile = (ctypes.c_int * 4)()
    assert _lib.load().dfh_nearest_descriptors_tile(tile) == 0
    assert list(tile) == [TILE_Q, TILE_B, EXACT_Q, SLOTS]


def run(q, b, path):
    _lib.set_option("nd_path", path)
    idx, d2, stats = solve.nearest_descriptors(q, b, return_d2=True, return_stats=True)
    return idx.cpu().numpy(), d2.cpu().numpy(), stats.cpu().numpy()


def check(q, b, path, what=None):
    """idx equal, d2 bit-equal to the restatement; returns (idx, d2, stats)."""
    idx, d2, stats = run(q, b, path)
    ridx, rd2 = DN.nearest_descriptors(q, b)
    assert idx.dtype == np.int32 and d2.dtype == np.float64
    assert np.array_equal(idx, ridx), (what, path, np.flatnonzero(idx != ridx)[:8])
    assert np.array_equal(d2.view(np.int64), rd2.view(np.int64)), (what, path)
    if path == 1:
        assert stats.tolist() == [0, len(q)]
    return idx, d2, stats


def edge_shapes(dim):
    rows = EXACT_FLOATS // dim
    shapes = [(1, 1), (1, 257), (257, 1), (2, 3)]
    for t in (MFMA, TILE_Q, EXACT_Q):                                # one below, at, one above each tile dimension, on both sides
        shapes += [(t - 1, t + 1), (t, t), (t + 1, t - 1)]
    shapes += [(TILE_Q + 5, TILE_B * 3 + 7)]                         # a ragged last tile on both sides, several chunks
    shapes += [(5, rows - 1), (5, rows), (5, rows + 1)]              # the exact kernel's staged chunk
    return shapes


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dim", [1, 3, 4, 16, 17, 64])
def test_shapes_at_the_kernels_edges(dim, path):
    rng = np.random.default_rng(100 + dim)
    for nq, nb in edge_shapes(dim):
        q = rng.standard_normal((nq, dim)).astype(np.float32)
        b = rng.standard_normal((nb, dim)).astype(np.float32)
        check(q, b, path, (dim, nq, nb))


def test_a_score_workgroup_walks_a_second_base_chunk():
    """nd_score_kernel's grid is (query tiles, base splits) with splits = min(ceil(2048 / query tiles), base chunks): a workgroup
    walks the chunks y, y + splits, ... and takes a second one only when query tiles x chunks > 2048.  8193 queries (65 tiles, the
    last of one query: 32 splits) against 4160 base rows (33 chunks, the last of 64 rows): the first split's workgroups reload
    their LDS chunk and carry their running minimum -- and, emitting, their candidate slots -- into chunk 32.  The fast path."""
    dim, nq, nb = 4, 64 * TILE_Q + 1, 32 * TILE_B + 64
    q_tiles, chunks = -(-nq // TILE_Q), -(-nb // TILE_B)
    splits = min(-(-2048 // q_tiles), chunks)
    assert (q_tiles, chunks, splits) == (65, 33, 32) and chunks > splits
    rng = np.random.default_rng(65)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    b = rng.standard_normal((nb, dim)).astype(np.float32)
    idx, _, _ = check(q, b, 2, (dim, nq, nb))
    assert (idx >= splits * TILE_B).sum() > 10                       # nearest rows in the chunk only the second turn reaches


@pytest.mark.parametrize("path", PATHS)
def test_exact_ties_go_to_the_lowest_index(path):
    rng = np.random.default_rng(7)
    b = rng.integers(0, 3, size=(300, 4)).astype(np.float32)         # 81 possible rows: every row has duplicates
    q = rng.integers(0, 3, size=(200, 4)).astype(np.float32)
    idx, d2, _ = check(q, b, path)
    full = DN.d2_matrix(q, b)
    assert ((full == d2[:, None]).sum(axis=1) >= 2).mean() > 0.8     # nearly every query's minimum is attained more than once
    assert np.array_equal(idx, np.array([np.flatnonzero(r == r.min())[0] for r in full]))
    # one distance for everything: index 0
    idx, d2, _ = check(np.zeros((70, 16), dtype=np.float32), np.ones((500, 16), dtype=np.float32), path)
    assert (idx == 0).all() and (d2 == 16.0).all()


def sub_ulp_case():
    """Base rows near 1000 that differ by single float32 ulps in single channels, queries within 1e-3 of them: the float32 scores
    of one query are (nearly) all the same number."""
    rng = np.random.default_rng(11)
    nb, dim, nq = 24, 16, 300
    b = np.full((nb, dim), 1000.0, dtype=np.float32)
    for l in range(nb):
        for _ in range(1 + l // dim):
            b[l, l % dim] = np.nextafter(b[l, l % dim], np.float32(2000.0))
    q = (b[rng.integers(0, nb, size=nq)].astype(np.float64) + rng.uniform(-1e-3, 1e-3, size=(nq, dim))).astype(np.float32)
    return q, b


def test_sub_ulp_case_defeats_the_f32_score():
    """The premise, in numpy: the float32 score cannot tell these base rows apart."""
    q, b = sub_ulp_case()
    s = DN.f32_scores(q, b)
    ridx, _ = DN.nearest_descriptors(q, b)
    assert (np.argmin(s, axis=1) == ridx).mean() < 0.05
    assert np.mean([len(np.unique(r)) for r in s]) < 2.0


@pytest.mark.parametrize("path", PATHS)
def test_ties_below_f32_resolution(path):
    q, b = sub_ulp_case()
    _, _, stats = check(q, b, path)
    if path == 2:                                                    # the guard band did the work: many rows per query re-evaluated
        assert stats[1] == 0
        assert stats[0] >= 8 * len(q), stats


@pytest.mark.parametrize("dim,nq,nb", [(16, 257, 1000), (3, 129, 257), (64, 65, 1000), (17, 64, 333)])
def test_the_filter_filters(dim, nq, nb):
    rng = np.random.default_rng(dim * 1000 + nq)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    b = rng.standard_normal((nb, dim)).astype(np.float32)
    _, _, stats = check(q, b, 2)
    assert stats[1] == 0 and nq <= stats[0] <= 2 * nq, stats


@pytest.mark.parametrize("path", PATHS)
def test_bad_and_large_values(path):
    rng = np.random.default_rng(23)
    dim, nq, nb = 16, 150, 300
    q0 = rng.standard_normal((nq, dim)).astype(np.float32)
    b0 = rng.standard_normal((nb, dim)).astype(np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        b = b0.copy()
        b[0] = q0[5]                                                 # would win query 5 outright ...
        b[0, 3] = bad                                                # ... but never counts
        b[17, 0] = bad
        idx, _, _ = check(q0, b, path, ("bad base row", bad))
        assert not np.isin(idx, [0, 17]).any() and (idx >= 0).all()
        q = q0.copy()
        q[3, 1] = bad
        q[149, 15] = bad
        idx, d2, stats = check(q, b0, path, ("bad query", bad))
        assert idx[3] == -1 and idx[149] == -1 and np.isposinf(d2[[3, 149]]).all() and (np.delete(idx, [3, 149]) >= 0).all()
        if path == 2:
            assert stats[1] == 2
        idx, d2, _ = check(q0, np.full((nb, dim), bad, dtype=np.float32), path, ("every base row bad", bad))
        assert (idx == -1).all() and np.isposinf(d2).all()
    b = b0.copy()
    b[:, 0] = np.nan                                                 # every base row bad through one channel
    idx, _, _ = check(q0, b, path)
    assert (idx == -1).all()
    # 1e20: float32 squares overflow, the definition's fp64 does not
    big = np.float32(1e20)
    idx, d2, stats = check(q0 * big, b0 * big, path, "1e20 on both sides")
    assert (idx >= 0).all() and np.isfinite(d2).all()
    if path == 2:
        assert stats.tolist() == [0, nq]
    q = q0.copy()
    q[7] *= big
    idx, _, stats = check(q, b0, path, "one query at 1e20")
    if path == 2:
        assert stats[1] == 1
    b = b0.copy()
    b[9] *= big
    check(q0, b, path, "one base row at 1e20")
    with np.errstate(over="ignore"):                                 # (most products are infinities: those queries get -1)
        top = q0 * np.float32(3e38)
    check(top, b0[:40], path, "queries at the top of float32")
    # float32 subnormals
    tiny = np.float32(1e-41)
    for n in (20, nb):
        qs, bs = (q0 * tiny).astype(np.float32), (b0[:n] * tiny).astype(np.float32)
        assert (np.abs(bs[bs != 0]) < np.finfo(np.float32).tiny).all()
        check(qs, bs, path, ("subnormals", n))
    check(q0, (b0 * tiny).astype(np.float32), path, "subnormal base, normal queries")


def _raw_call(q, b, path, want_d2=True, want_stats=True, guard=8):
    """The C entry point with guard words behind idx_out and d2_out."""
    lib = _lib.load()
    _lib.set_option("nd_path", path)
    nq, nb, dim = q.shape[0], b.shape[0], q.shape[1]
    idx = torch.full((nq + guard,), -12345, dtype=torch.int32, device="cuda")
    d2 = torch.full((nq + guard,), -7.5, dtype=torch.float64, device="cuda")
    stats = torch.full((2 + guard,), -99, dtype=torch.int64, device="cuda")
    nbytes = lib.dfh_nearest_descriptors_workspace_bytes(nq, nb, dim)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.dfh_nearest_descriptors(q.data_ptr(), nq, b.data_ptr(), nb, dim, idx.data_ptr(), d2.data_ptr() if want_d2 else 0,
                                           stats.data_ptr() if want_stats else 0, ws.data_ptr(), nbytes, current_stream_ptr()),
               "dfh_nearest_descriptors")
    torch.cuda.synchronize()
    return idx, d2, stats


@pytest.mark.parametrize("path", PATHS)
def test_determinism_and_containment(path):
    rng = np.random.default_rng(31)
    nq, nb, dim = 1000, 3001, 16
    qn = rng.standard_normal((nq, dim)).astype(np.float32)
    bn = rng.standard_normal((nb, dim)).astype(np.float32)
    bn[100:140] = bn[99]                                             # 41 equal rows: more candidates than slots for their queries
    qn[:10] = bn[99] + np.float32(0.001)
    qn[20, 0] = np.nan
    q, b = torch.from_numpy(qn).cuda(), torch.from_numpy(bn).cuda()
    ridx, rd2 = DN.nearest_descriptors(qn, bn)
    a = _raw_call(q, b, path)
    c = _raw_call(q, b, path)
    for x, y in zip(a, c):
        assert torch.equal(x, y)
    idx, d2, stats = a
    assert np.array_equal(idx[:nq].cpu().numpy(), ridx) and np.array_equal(d2[:nq].cpu().numpy().view(np.int64), rd2.view(np.int64))
    assert (idx[nq:] == -12345).all() and (d2[nq:] == -7.5).all() and (stats[2:] == -99).all()
    if path == 2:
        assert stats[1].item() == 11                                 # the ten queries beside the 41 equal rows, and the NaN
    idx2, d2b, st2 = _raw_call(q, b, path, want_d2=False, want_stats=False)
    assert torch.equal(idx2, idx) and (d2b == -7.5).all() and (st2 == -99).all()
    # the Python wrapper: float32-exact float64 and tensors pass, the results are the same
    i3 = solve.nearest_descriptors(qn.astype(np.float64), b)
    assert torch.equal(i3, idx[:nq])
    assert solve.nearest_descriptors(np.zeros((0, dim), dtype=np.float32), bn).shape == (0,)


def test_default_path_gives_the_same_bits():
    rng = np.random.default_rng(37)
    q = rng.standard_normal((2100, 16)).astype(np.float32)
    b = rng.standard_normal((2100, 16)).astype(np.float32)
    for n in (40, 2100):                                             # either side of whatever the library's threshold is
        assert _lib.load().dfh_nearest_descriptors_path(n, n, 16) in (1, 2)
        check(q[:n], b[:n], None)


# ---- the Fusion layer ------------------------------------------------------------------------------------------------------------
R = 64
CENTRE = np.array([31.3, 32.4, 31.8])
RNG_MAP = np.random.default_rng(5).standard_normal((3, 16))          # descriptors = a fixed linear map of the MATERIAL point


def _grid():
    return np.meshgrid(*(np.arange(R, dtype=np.float64),) * 3, indexing="ij")


def _rot_z(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _ellipsoid_sdf(axes, rot=np.eye(3), shift=np.zeros(3)):
    """An approximate signed distance (in voxels, clipped to +-3) of an ellipsoid about CENTRE, moved by x -> rot (x - c) + c + shift."""
    X, Y, Z = _grid()
    P = np.stack([X, Y, Z], axis=-1) - CENTRE - shift
    P = P @ rot                                                       # rot^T applied to the rows: back into the body's frame
    k = np.sqrt(((P / axes) ** 2).sum(axis=-1))
    return np.clip((k - 1.0) * axes.min(), -3.0, 3.0).astype(np.float32)


def _features(points):
    return (np.asarray(points, dtype=np.float64) @ RNG_MAP).astype(np.float32)


def _preimage(points, rot, shift):
    return (np.asarray(points, dtype=np.float64) - CENTRE - shift) @ rot + CENTRE


def _fusion(canon, lw=None):
    fu = Fusion(canon, 3.0, subsample_rate=3.0, knn=4, marching_cubes_step_size=3, write_warpfield=False)
    fu._lw = np.array([1.0, 0, 0, 0, 0, 0, 0, 0]) if lw is None else lw
    fu.initialize_canonical()
    return fu


def _restate_cnn_branch(fu0, lverts, s_feats, l_feats, prune, tolerance):
    """core/fusion.py:277-313 in numpy on the state of the un-called Fusion `fu0`: (correspondences, keep, node anchors, costs)."""
    V = np.asarray(fu0._vertices, dtype=np.float64)
    Nn = np.asarray(fu0._normals, dtype=np.float64)
    nbr = np.asarray(fu0._neighbor_look_up)
    pos, dq, w, _ = fu0.node_arrays()
    idx, _ = DN.nearest_descriptors(s_feats, l_feats)
    vp, wn = O.warp(V, dq[nbr], pos[nbr], w[nbr], normal=Nn, m_lw=np.asarray(fu0._lw, dtype=np.float64))
    corr = np.where((idx >= 0)[:, None], np.asarray(lverts, dtype=np.float64)[np.maximum(idx, 0)], vp)
    d = vp - corr
    cost = np.abs((wn[:, 0] * d[:, 0] + wn[:, 1] * d[:, 1]) + wn[:, 2] * d[:, 2])
    keep = (idx >= 0) & ~(cost > tolerance) if prune else np.ones(len(V), dtype=bool)
    anchors = []
    for p in pos:                                                    # dfh_nearest_points: squared distances, the lowest index on ties
        e = V[keep] - p
        anchors.append(int(np.argmin((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])))
    return corr, keep, anchors, cost


@pytest.fixture(scope="module")
def fusion_scene():
    axes = np.array([19.0, 14.0, 11.0])
    rot, shift = _rot_z(0.2), np.array([0.6, -0.4, 0.3])
    canon, live = _ellipsoid_sdf(axes), _ellipsoid_sdf(axes, rot, shift)
    lw = G.twist_exp_dq(np.array([0.01, -0.02, 0.015, 0.2, -0.1, 0.15]))
    probe = _fusion(canon, lw)
    lverts = probe.marching_cubes(live, step_size=1)[0]
    s_feats = _features(probe._vertices)
    l_feats = _features(_preimage(lverts, rot, shift))
    l_feats[3] = np.nan                                              # a live vertex nothing may be matched with
    return dict(canon=canon, live=live, lw=lw, rot=rot, shift=shift, lverts=lverts, s_feats=s_feats, l_feats=l_feats)


@pytest.mark.parametrize("path", PATHS)
def test_fusion_cnn_branch_matches_the_restatement(fusion_scene, path):
    sc = fusion_scene
    _lib.set_option("nd_path", path)
    fu0 = _fusion(sc["canon"], sc["lw"])
    nv = len(fu0._vertices)
    assert nv > 300 and len(sc["lverts"]) > 5 * nv
    s_feats = sc["s_feats"].copy()
    s_feats[11] = np.inf                                             # a canonical vertex without a comparable descriptor: index -1
    _, _, _, cost = _restate_cnn_branch(fu0, sc["lverts"], s_feats, sc["l_feats"], False, 0.0)
    # a tolerance that splits the vertices, in the widest gap of the sorted costs around the median (the device's warp agrees
    # with the oracle's to 1e-12, the existing bar of warp_points: no cost may sit that close to the tolerance)
    cs = np.sort(cost[np.arange(nv) != 11])
    mid = len(cs) // 2
    k = mid - 20 + int(np.argmax(np.diff(cs[mid - 20:mid + 20])))
    tol = 0.5 * (cs[k] + cs[k + 1])
    assert cs[k + 1] - cs[k] > 1e-9
    # without pruning: every vertex keeps a correspondence, the -1 vertex its own warped position
    corr, keep, anchors, _ = _restate_cnn_branch(fu0, sc["lverts"], s_feats, sc["l_feats"], False, tol)
    fu = _fusion(sc["canon"], sc["lw"])
    fu.setupCorrespondences(sc["live"], method='cnn', prune_result=False, tolerance=tol, descriptors=(s_feats, sc["l_feats"]))
    C = np.asarray(fu._correspondences)
    assert len(fu._vertices) == nv and C.shape == (nv, 3)
    assert np.array_equal(np.delete(C, 11, axis=0), np.delete(corr, 11, axis=0))
    assert np.abs(C[11] - corr[11]).max() <= 1e-12
    assert not (C == np.asarray(sc["lverts"], dtype=np.float64)[3]).all(axis=1).any()
    # with pruning: the kept set, the bookkeeping and the re-anchored nodes
    corr, keep, anchors, _ = _restate_cnn_branch(fu0, sc["lverts"], s_feats, sc["l_feats"], True, tol)
    assert 0.25 * nv < keep.sum() < 0.75 * nv and not keep[11]
    fu = _fusion(sc["canon"], sc["lw"])
    fu.setupCorrespondences(sc["live"], method='cnn', prune_result=True, tolerance=tol, descriptors=(s_feats, sc["l_feats"]))
    assert np.array_equal(fu._vertices, np.asarray(fu0._vertices)[keep]) and np.array_equal(fu._normals, np.asarray(fu0._normals)[keep])
    assert np.array_equal(fu._neighbor_look_up, np.asarray(fu0._neighbor_look_up)[keep])
    assert np.array_equal(np.asarray(fu._correspondences), corr[keep]) and fu._faces is None
    assert [int(nd[0]) for nd in fu._nodes] == anchors and all(nd[3] == 2 * fu._radius for nd in fu._nodes)
    # explicit live vertices in place of the marching-cubes call: the same result
    fv = _fusion(sc["canon"], sc["lw"])
    fv.setupCorrespondences(None, method='cnn', prune_result=True, tolerance=tol, descriptors=(s_feats, sc["l_feats"]),
                            live_vertices=sc["lverts"])
    assert np.array_equal(np.asarray(fv._correspondences), np.asarray(fu._correspondences))


def test_descriptor_fn_equals_the_explicit_pair_and_cnn_without_either_is_closest_points(fusion_scene):
    sc = fusion_scene
    fa = _fusion(sc["canon"], sc["lw"])
    fa.setupCorrespondences(sc["live"], method='cnn', prune_result=True, tolerance=1.0, descriptors=(sc["s_feats"], sc["l_feats"]))
    calls = []

    def descriptor_fn(vertices, faces):
        calls.append((len(vertices), None if faces is None else len(faces)))
        if len(calls) == 1:                                          # the canonical mesh first (core/fusion.py:280), then the live one
            return _features(vertices)
        f = _features(_preimage(vertices, sc["rot"], sc["shift"]))
        f[3] = np.nan
        return f
    fb = _fusion(sc["canon"], sc["lw"])
    fb.descriptor_fn = descriptor_fn
    fb.setupCorrespondences(sc["live"], method='cnn', prune_result=True, tolerance=1.0)
    assert len(calls) == 2 and calls[0][1] is not None and calls[1] == (len(sc["lverts"]), calls[1][1]) and calls[1][1] > 0
    assert np.array_equal(np.asarray(fa._correspondences), np.asarray(fb._correspondences))
    assert np.array_equal(fa._vertices, fb._vertices) and [n[0] for n in fa._nodes] == [n[0] for n in fb._nodes]
    assert 0 < len(fa._vertices) < len(sc["s_feats"])
    # neither a pair nor a callable: the closest-points branch, as before
    fc, fd = _fusion(sc["canon"], sc["lw"]), _fusion(sc["canon"], sc["lw"])
    fc.setupCorrespondences(sc["live"], method='cnn', prune_result=True, tolerance=0.2)
    fd.setupCorrespondences(sc["live"], method='clpts', prune_result=True, tolerance=0.2)
    assert np.array_equal(np.asarray(fc._correspondences), np.asarray(fd._correspondences))
    assert np.array_equal(fc._vertices, fd._vertices) and [n[0] for n in fc._nodes] == [n[0] for n in fd._nodes]
    assert not np.array_equal(np.asarray(fc._vertices), np.asarray(fa._vertices))


# ---- what it buys ---------------------------------------------------------------------------------------------------------------
def _angle_z(lw):
    M = O.DQTSE3(np.asarray(lw, dtype=np.float64))
    return float(np.arctan2(M[1, 0], M[0, 0]))


def _rigid_prefit_np(V, Nn, C, iters=10):
    x = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
    for _ in range(iters):
        x, _, _ = G.gn_step_rigid(x, V, Nn, C)
    return x


def test_descriptors_recover_a_turn_about_the_axis():
    """A sphere turned about its own axis by 0.15 rad: the live volume IS the canonical volume, so closest points (and every
    other proximity association) sees a motion of zero; descriptors that follow the material point see the turn.  The `_lw`
    pre-fit of solve() from both sets of correspondences, against the numpy restatement (the nearest-descriptor search of
    tests/descriptors_np.py or the oracle's closest points, then ten oracle Gauss-Newton steps) at the rigid solve's bar, and
    the restatement's two angles against the recorded ones (tests/golden/descriptor_recovery.json)."""
    theta = 0.15
    rot = _rot_z(theta)
    vol = _ellipsoid_sdf(np.array([20.0, 20.0, 20.0]))
    got, want = {}, {}
    for method in ("cnn", "clpts"):
        fu = _fusion(vol)
        # an undeformed graph (new nodes carry the reference's 0.02-voxel translation): the blend warp is then the identity,
        # the pre-fit's points are the vertices themselves and the restatement needs no graph
        fu._nodes = [(nd[0], nd[1], np.array([1.0, 0, 0, 0, 0, 0, 0, 0]), nd[3]) for nd in fu._nodes]
        V, Nn = np.asarray(fu._vertices, dtype=np.float64), np.asarray(fu._normals, dtype=np.float64)
        lverts = fu.marching_cubes(vol, step_size=1)[0]
        if method == "cnn":
            pair = (_features(V), _features(_preimage(lverts, rot, np.zeros(3))))
            fu.setupCorrespondences(vol, method='cnn', prune_result=False, descriptors=pair)
            idx, _ = DN.nearest_descriptors(*pair)
            C = np.asarray(lverts, dtype=np.float64)[idx]
        else:
            fu.setupCorrespondences(vol, method='clpts', prune_result=False)
            C, _, _ = O.closest_correspondences(V, Nn, lverts, fu._knn, 0.2)
        assert np.array_equal(np.asarray(fu._correspondences), C)
        fu.solve(correspondences=fu._correspondences, method=method, precompute_lw=True, iterations=10)
        x = _rigid_prefit_np(V, Nn, C, 10)
        assert np.abs(np.asarray(fu._lw) - x).max() <= 1e-9, method
        got[method], want[method] = _angle_z(fu._lw), _angle_z(x)
    rec = json.load(open(GOLDEN))
    print("recovered angle about z: descriptors %.9f, closest points %.9f (true %.2f)" % (want["cnn"], want["clpts"], theta))
    assert rec["theta"] == theta
    for method in ("cnn", "clpts"):
        assert abs(got[method] - want[method]) <= 1e-9
        assert abs(want[method] - rec["angle_z_" + method]) <= 1e-6, (method, want[method], rec)
