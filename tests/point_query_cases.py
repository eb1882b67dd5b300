"""Inputs for the point-query and graph kernels at their decision boundaries (tests/test_point_query_fixtures.py on the CPU,
tests/test_gpu_point_queries.py on the GPU): dfh_closest_correspondences, dfh_nearest_points, dfh_graph_unsupported,
dfh_dq_blend_points, dfh_warp_points, dfh_residual_data / _reg, dfh_sample_knn.

Every case is generated from the constants below (nothing here is a golden file) and is built so that the numpy oracle ALONE is
unambiguous: the oracle uses the kernels' operation order ((a + b) + c, no contraction), ties are resolved by stable order, and the
crafted rows use dyadic numbers with few bits, for which every operation of the chain is exact -- a cost of exactly 1, a cost
exactly equal to the tolerance, a ratio of exactly 1 and a blend of exactly 0 are what they say in any summation order.
Coordinates stay inside [-5, 60] like everywhere in the suite.

A case carries `rows`: name -> indices of the rows crafted for that boundary; the CPU test proves through the oracle that each of
them is what it claims, so a later change of a generator cannot move off a boundary without a failure."""
import numpy as np

from oracle import oracle_np as O

TILE = 256                                          # rows per workgroup, and rows per LDS tile of the live cloud
KNNS = tuple(range(1, 9))
TOLERANCES = (0.2, 0.25, 1.0)                       # 0.25: the dyadic twin of 0.2 (a cost of exactly the tolerance is kept)


def _grid(rng, n, lo, hi, step):
    """n x 3 random multiples of `step` (a power of two) in [lo, hi]."""
    return rng.integers(int(lo / step), int(hi / step) + 1, size=(n, 3)).astype(np.float64) * step


def _pair(n, a, b):
    """(a, b) when the cloud holds both, else the last two indices; None for a cloud of one."""
    if n > b:
        return a, b
    return (n - 2, n - 1) if n >= 2 else None


# ------------------------------------------------------------------------------------------------ dfh_closest_correspondences
def closest_live_sizes(knn):
    return sorted({knn, 255, 256, 257, 513})


CLOSEST_VERTS = (1, 255, 256, 257)


def closest_case(knn, n_live, n_verts, nonfinite=False):
    """Live vertices on the 1/8 grid of [0, 40]^3 (every squared distance exact, many natural distance ties between different
    points), with exact duplicates -- one pair across the LDS tile boundary (255, 256) -- and crafted points around x = 50..57
    that the crafted rows (the first ones) look at.  Rows beyond the crafted ones alternate between grid points (exact ties) and
    generic doubles (rounding: the oracle's operation order is the kernel's).
    nonfinite: additionally rows whose position is NaN / +inf / -inf in one coordinate (after the crafted ones)."""
    rng = np.random.default_rng(1000 * knn + n_live)
    n = n_live
    live = _grid(rng, n, 0.0, 40.0, 0.125)
    rows = {}
    # exact duplicates (the same coordinates twice): first against last, neighbours inside a tile, across the tile boundary
    dups = ([(0, n - 1)] if n >= 4 and n != 257 else []) + ([(1, 2)] if n >= 6 else []) + ([(255, 256)] if n >= 257 else [])
    for a, b in dups:
        live[b] = live[a]
    # "tile_tie": two DIFFERENT live points at the same distance from a row and with the same cost, on either side of the tile
    # boundary when the cloud has 258 points or more: the lower index is the nearest (knn = 1) and the first of equal costs
    tp = (254, 257) if n >= 258 else (250, 254) if n == 257 else (n - 3, n - 2) if n >= 4 else (0, 1) if n >= 2 else None
    taken = {i for p in dups for i in p} | set(tp or ())
    free = [i for i in range(n) if i not in taken]

    def put(xyz):
        """A crafted live point into a free slot, from either end of the cloud in turn (the first and the last tile)."""
        if not free:
            return False
        live[free.pop(0 if len(free) % 2 else -1)] = xyz
        return True

    crafted_pos, crafted_nrm = [], []

    def row(name, pos, nrm):
        rows.setdefault(name, []).append(len(crafted_pos))
        crafted_pos.append(np.asarray(pos, dtype=np.float64)); crafted_nrm.append(nrm)

    if tp is not None:
        c = np.array([50.0, 50.0, 8.0])
        live[tp[0]], live[tp[1]] = c + [0.5, 0.0, 0.0], c - [0.5, 0.0, 0.0]
        row("tile_tie", c, [0.25, 0.0, 0.0])                                          # cost 0.125 for both
    # "all_ge_1": x on an odd multiple of 1/16, every live x a multiple of 1/8, normal (16, 0, 0) or (1024, 0, 0): every cost is an
    # odd integer or more; "cost_1": the nearest live point sits at dx = -1/16: its cost is exactly 1, not below the initial best_cost
    q = np.array([56.0 + 1.0 / 16, 20.0, 20.0])
    if put(q + [1.0 / 16, 0.0, 0.0]):
        rows["cost_1"] = [len(crafted_pos)]
    row("all_ge_1", q, [16.0, 0.0, 0.0])
    row("all_ge_1", q + [0.0, 0.25, 0.0], [1024.0, 0.0, 0.0])
    # "cost_eq_tol": the nearest live point at d = (1, 0, 0), normal (t, 0, 0): cost = (t * 1 + 0) + 0 = t exactly, for t = 0.2 (the
    # tolerance's own double) and for the dyadic 0.25: kept; "cost_above_tol": t = the next double above: not kept
    q = np.array([52.0, 4.0, 30.0])
    if put(q - [1.0, 0.0, 0.0]):
        for t in (0.2, 0.25):
            row("cost_eq_tol", q, [t, 0.0, 0.0])
            row("cost_above_tol", q, [np.nextafter(t, 1.0), 0.0, 0.0])
    # "nan_normal": a finite position with a NaN normal: no cost compares below 1 -> best = nearest, cost = 1
    row("nan_normal", [10.0625, 10.0, 10.0], [np.nan, 0.5, 0.0])
    # "dup": rows right next to the duplicated live points
    for a, b in dups:
        row("dup", live[a] + [0.0625, 0.0, -0.0625], [0.125, -0.25, 0.0625])
    if nonfinite:
        for bad in ([np.nan, 3.0, 4.0], [1.0, np.inf, 2.0], [5.0, 6.0, -np.inf], [np.nan, np.nan, np.nan]):
            row("nonfinite", bad, [0.25, 0.0, 0.0])
    crafted_pos, crafted_nrm = np.array(crafted_pos), np.array(crafted_nrm, dtype=np.float64)
    # the rest: grid rows with small dyadic normals (costs below and above 1, equal costs) / generic rows
    n_rest = max(0, n_verts - len(crafted_pos))
    gp, gn = _grid(rng, n_rest, -5.0, 45.0, 0.0625), _grid(rng, n_rest, -0.25, 0.25, 1.0 / 64)
    up, un = rng.uniform(-5.0, 45.0, size=(n_rest, 3)), rng.normal(size=(n_rest, 3)) * 0.05
    odd = (np.arange(n_rest) % 2 == 1)[:, None]
    pos = np.concatenate([crafted_pos, np.where(odd, up, gp)])[:n_verts]
    nrm = np.concatenate([crafted_nrm, np.where(odd, un, gn)])[:n_verts]
    rows = {name: [i for i in idx if i < n_verts] for name, idx in rows.items()}
    return dict(knn=knn, live=live, pos=np.ascontiguousarray(pos), nrm=np.ascontiguousarray(nrm), rows=rows, dups=dups, tile_pair=tp)


# ------------------------------------------------------------------------------------------------ dfh_nearest_points
NEAREST_CLOUDS = (1, 255, 256, 257, 1000)
NEAREST_QUERIES = (1, 3, 300)


def nearest_case(n_cloud, n_query, nonfinite=False):
    """Generic doubles (d2 must be bit-equal: same operations in the same order).  The kernel gives thread t the points t,
    t + 256, ... and reduces the 256 threads' (d2, index) pairs: the first queries sit on exact ties between
      cross   a lower index held by a HIGHER thread (5 against 258 = thread 2; 3 against 256 = thread 0): the reduction's tie-break,
      same    two indices of the same thread (44 and 300): the strict < of the thread's own scan,
      next    neighbouring threads (10, 11), mirrored about a dyadic query instead of duplicated.
    ties: query -> (lower, higher index), the lower one is the answer."""
    rng = np.random.default_rng(7 * n_cloud + n_query)
    cloud = rng.uniform(0.0, 40.0, size=(n_cloud, 3))
    query = rng.uniform(-5.0, 45.0, size=(n_query, 3))
    n = n_cloud
    cross = (5, 258) if n >= 259 else (3, 256) if n >= 257 else (5, 200) if n >= 201 else None
    same = (44, 300) if n >= 301 else None
    nxt = (10, 11) if n >= 12 else None
    ties = {}
    qi = 0
    for pair in (cross, same):
        if pair is not None and qi < n_query:
            cloud[pair[1]] = cloud[pair[0]]
            query[qi] = cloud[pair[0]] + [0.03, -0.02, 0.01]
            ties[qi] = pair
            qi += 1
    if nxt is not None and qi < n_query:
        q = np.array([48.0, 50.0, 52.0])
        cloud[nxt[0]], cloud[nxt[1]] = q + [0.25, -0.5, 0.125], q - [0.25, -0.5, 0.125]
        query[qi] = q
        ties[qi] = nxt
        qi += 1
    if n_query > qi + 4:
        query[qi:qi + 4] = cloud[rng.integers(0, n_cloud, size=4)]                 # on a cloud point: d2 = 0
    bad = []
    if nonfinite and n_query >= 8:
        bad = [n_query - 1, n_query - 3, n_query - 5]
        query[bad[0]] = [np.nan, 1.0, 2.0]; query[bad[1]] = [3.0, -np.inf, 2.0]; query[bad[2]] = [np.inf, np.nan, 0.0]
    return dict(cloud=cloud, query=query, ties=ties, nonfinite=bad)


# ------------------------------------------------------------------------------------------------ dfh_graph_unsupported
GRAPH_VERTS = (255, 256, 257)
N_NODES = 40


def _graph_nodes(rng, n=N_NODES):
    """n nodes on the 1/4 grid of [8, 40]^3, weights 2 .. 6 (dyadic)."""
    return _grid(rng, n, 8.0, 40.0, 0.25), rng.integers(8, 25, size=n).astype(np.float64) * 0.25


def unsupported_case(knn, n_verts):
    """Random vertices with random node lists (the kernel takes the lists as they come), and crafted rows around node 0 (weight 5):
      at_1      the vertex at offset (3, 4, 0) permutations from the node: |d| = sqrt(25) = 5 exactly, ratio exactly 1: flagged;
      inside    the same with the 4 shortened by one ulp of the coordinate: ratio just below 1: not flagged;
      inside_w  offset (3, 4, 0) from node 1, whose weight is the next double above 5;
    every other node of such a row is far away (ratio > 1), and the crafted node takes every position of the list in turn."""
    rng = np.random.default_rng(50 * knn + n_verts)
    npos, nw = _graph_nodes(rng)
    npos[0], nw[0] = [24.0, 24.0, 24.0], 5.0
    npos[1], nw[1] = [24.0, 24.0, 48.0], np.nextafter(5.0, 6.0)
    npos[2:6] = [[56.0, 0.0, 0.0], [0.0, 56.0, 0.0], [56.0, 56.0, 0.0], [0.0, 0.0, 2.0]]     # the far nodes of the crafted rows
    nw[2:6] = 2.0
    verts = rng.uniform(0.0, 48.0, size=(n_verts, 3))
    nbr = rng.integers(0, N_NODES, size=(n_verts, knn)).astype(np.int32)
    rows = dict(at_1=[], inside=[], inside_w=[])
    offs = [(3.0, 4.0, 0.0), (0.0, -3.0, 4.0), (-4.0, 0.0, 3.0), (4.0, 3.0, 0.0), (0.0, 4.0, -3.0), (-3.0, 0.0, -4.0), (3.0, -4.0, 0.0), (0.0, 3.0, 4.0)]
    r = 0
    for slot in range(knn):
        far = np.array([2 + (j + slot) % 4 for j in range(knn)], dtype=np.int32)
        for name in ("at_1", "inside", "inside_w"):
            off = np.array(offs[(slot + len(rows[name])) % len(offs)])
            node = 1 if name == "inside_w" else 0
            v = npos[node] + off
            if name == "inside":
                ax = int(np.argmax(np.abs(off)))                     # the coordinate that carries the 4: one ulp towards the node
                v[ax] = np.nextafter(v[ax], npos[node][ax])
            verts[r] = v
            nbr[r] = far
            nbr[r, slot] = node
            rows[name].append(r)
            r += 1
    return dict(knn=knn, verts=verts, nbr=nbr, node_pos=npos, node_w=nw, rows=rows)


# ------------------------------------------------------------------------------------------------ the warp family
def unit_dqs(rng, n, angle=0.6, shift=3.0):
    """n unit dual quaternions: a rotation of up to ~angle rad about a random axis, then a translation of up to ~shift."""
    ax = rng.normal(size=(n, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    th = rng.uniform(-angle, angle, size=n)
    qr = np.concatenate([np.cos(th / 2)[:, None], np.sin(th / 2)[:, None] * ax], axis=1)
    t = np.concatenate([np.zeros((n, 1)), rng.uniform(-shift, shift, size=(n, 3))], axis=1)
    qd = 0.5 * O.quaternion_multiply(t, qr)
    return np.concatenate([qr, qd], axis=1)


def blend_case(knn, n_points=257):
    """dfh_dq_blend_points: random points with random node lists, and crafted rows
      underflow  so far from all their nodes (nodes 2..9: weight 1/4, 60 and more away) that every weight exp(-(d / 2w)^2) is
                 exactly 0: the identity;
      cancel     (knn >= 2) nodes 0 and 1 carry q and -q, have the same weight and sit mirrored about the point: the two weights
                 are the same double and the blend is exactly 0 (an odd knn fills up with a node that underflows): the identity."""
    rng = np.random.default_rng(300 + knn)
    npos, nw = _graph_nodes(rng)
    ndq = unit_dqs(rng, N_NODES)
    npos[2:10] = _grid(rng, 8, -5.0, -1.0, 0.25)
    nw[2:10] = 0.25
    p = np.array([30.0, 20.0, 10.0])
    npos[0], npos[1] = p + [1.5, -0.75, 2.0], p - [1.5, -0.75, 2.0]
    nw[0] = nw[1] = 3.0
    ndq[1] = -ndq[0]
    pts = rng.uniform(0.0, 45.0, size=(n_points, 3))
    nbr = rng.integers(10, N_NODES, size=(n_points, knn)).astype(np.int32)
    rows = dict(underflow=[0, 1, TILE - 1, TILE], cancel=[])
    for r in rows["underflow"]:
        pts[r] = [58.0, 59.0, 60.0 - 0.5 * (r % 3)]
        nbr[r] = 2 + (np.arange(knn) + r) % 8
    if knn >= 2:
        rows["cancel"] = [2, 3, TILE - 2]
        for r in rows["cancel"]:
            pts[r] = p
            row = [(j + r) % 2 for j in range(knn - knn % 2)] + [2 + r % 8] * (knn % 2)
            nbr[r] = row if r != 3 else row[::-1]
    return dict(knn=knn, pts=pts, nbr=nbr, node_pos=npos, node_w=nw, node_dq=ndq, rows=rows)


def warp_case(knn, n_verts):
    """dfh_warp_points / dfh_residual_data / dfh_residual_reg: n_verts vertices AND n_verts nodes (the regulariser launches a thread
    per node and neighbour), positions and normals generic doubles -- none of them a float32 number, so that a missing round to
    float32 (core/util.py:69) shows as ~1e-6.  nbr: the knn nearest nodes; node_nbr: the nodes' own nearest nodes, themselves included on every other row."""
    rng = np.random.default_rng(9000 + 10 * knn + n_verts)
    N = n_verts
    npos = rng.uniform(5.0, 45.0, size=(N, 3))
    nw = rng.uniform(2.0, 6.0, size=N)
    ndq = unit_dqs(rng, N, angle=0.08, shift=0.5)
    verts = rng.uniform(0.0, 50.0, size=(n_verts, 3))
    nrm = rng.normal(size=(n_verts, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    corr = verts + rng.normal(size=(n_verts, 3)) * 0.3
    lw = unit_dqs(rng, 1, angle=0.05, shift=0.5)[0]
    near = O.knn_bruteforce(npos, npos, knn + 1)                       # column 0: the node itself
    node_nbr = np.where((np.arange(N) % 2 == 0)[:, None], near[:, :knn], near[:, 1:])      # with and without itself (a row of zeros)
    return dict(knn=knn, verts=verts, nrm=nrm, corr=corr, lw=lw, node_pos=npos, node_w=nw, node_dq=ndq,
                nbr=O.knn_bruteforce(verts, npos, knn).astype(np.int32), node_nbr=node_nbr.astype(np.int32))


# ------------------------------------------------------------------------------------------------ dfh_sample_knn, non-finite samples
def sample_knn_case(n_nodes, knn, n_samples=600):
    """Spatially coherent samples (the kernel prunes the nodes by the workgroup's bounding box) with non-finite ones among them:
    NaN, +inf and -inf coordinates in the first workgroup, an all-NaN row in the second, the third workgroup clean.  `finite`: the
    same samples with the non-finite rows replaced by ordinary points."""
    rng = np.random.default_rng(n_nodes + knn)
    npos = rng.uniform(0.0, 1.0, size=(n_nodes, 3)) * [31.0, 39.0, 47.0]      # inside the grid the brick-list test uses
    npos[n_nodes // 2] = npos[n_nodes // 3]
    nw = rng.uniform(2.0, 6.0, size=n_nodes)
    z = np.arange(n_samples, dtype=np.float64)
    finite = np.stack([20.0 + (z // 300) + 0.3 * np.sin(z), 33.0 + 0.2 * np.cos(z), (z % 300) * 0.2], axis=1)
    pts = finite.copy()
    bad = [3, 64, 200, TILE + 17]
    pts[3, 0] = np.nan; pts[64, 1] = np.inf; pts[200, 2] = -np.inf; pts[TILE + 17] = np.nan
    return dict(knn=knn, node_pos=npos, node_w=nw, pts=pts, finite=finite, nonfinite=bad)


# ------------------------------------------------------------------------------------------------ dfh_gn_pack_upper / _unpack_upper
def block_system(rng, rows, col, n_nodes, symmetric):
    """A flat system {blocks (B x 36) | J^T r (6 N) | cost, count} on the pattern (rows, col): symmetric -> block (b, a) is the
    transpose of block (a, b) and the diagonal blocks are symmetric; else every entry is its own random number."""
    B = len(col)
    blocks = rng.normal(size=(B, 6, 6))
    if symmetric:
        where = {(int(r), int(c)): b for b, (r, c) in enumerate(zip(rows, col))}
        for (r, c), b in where.items():
            if c < r:
                blocks[b] = blocks[where[(c, r)]].T
            elif c == r:
                blocks[b] = np.triu(blocks[b]) + np.triu(blocks[b], 1).T
    return np.concatenate([blocks.reshape(-1), rng.normal(size=6 * n_nodes), [rng.uniform(1, 2), float(B)]])
