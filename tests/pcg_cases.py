"""Systems for the block-Jacobi PCG at its launch shapes, row widths and degenerate blocks (tests/test_pcg_cases.py on the CPU,
tests/test_gpu_pcg_shapes.py on the GPU).

Every system is a Gram matrix: rows of a sparse Jacobian, each touching a few nodes with a 1 x 6 piece per node, A = sum J^T J as
6x6 blocks in the device's CSR layout (row_ptr, col ascending, vals) with keys = row * N + col for the oracle, rhs = J^T r.  Every
node has an explicit diagonal block, all zero if no row touches it.  Such a system is positive semi-definite at any size without
an eigen-decomposition, and with the bench's damping ten block-Jacobi PCG iterations leave it far from converged (a diagonally
dominant random matrix converges in ten and says nothing about the truncated iterate).

A case names what it is there for in `claims`; test_pcg_cases.py asserts each claim on the inputs, so a later change of a case
cannot move off the launch shape, the row width or the diagonal position it was made for without a failure.  Nothing here is a
golden file: everything is generated from the constants below."""
import functools

import numpy as np

LM = (10.0, 1e-2)                        # the bench's damping (lm_abs, lm_rel)
LM_WEAK = (1e-3, 1e-2)
OFFSETS = (0, 1, 2, 5)                   # a standard row touches nodes a + OFFSETS (mod the ring's length)
ROWS_PER_NODE = 12
ITERS = (1, 2, 3, 4, 5, 10)              # the iteration counts every case is compared at
ROW_CACHE = 30                           # blocks of a row the persistent kernel keeps in registers (kRowCache x 10 lane slots)


def _reduce_by_key(keys, vals):
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    start = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    return ks[start], np.add.reduceat(vals[order], start, axis=0)


def gram_system(N, groups):
    """groups: list of (nodes (S, k) int, J (S, k, 6), r (S,)).  Returns dict(N, keys, blocks, Jtr, row_ptr, col)."""
    key_parts = [np.arange(N, dtype=np.int64) * (N + 1)]
    blk_parts = [np.zeros((N, 6, 6))]
    Jtr = np.zeros((N, 6))
    for nodes, J, r in groups:
        nodes = np.asarray(nodes, dtype=np.int64)
        for a in range(nodes.shape[1]):
            np.add.at(Jtr, nodes[:, a], J[:, a, :] * r[:, None])
            for b in range(nodes.shape[1]):
                kk, bb = _reduce_by_key(nodes[:, a] * N + nodes[:, b], J[:, a, :, None] * J[:, b, None, :])
                key_parts.append(kk)
                blk_parts.append(bb)
    keys, blocks = _reduce_by_key(np.concatenate(key_parts), np.concatenate(blk_parts))
    rows = keys // N
    mirror = np.searchsorted(keys, (keys % N) * N + rows)                  # exactly symmetric, whatever order the sums ran in
    blocks = 0.5 * (blocks + np.transpose(blocks[mirror], (0, 2, 1)))
    return dict(N=N, keys=keys, blocks=blocks, Jtr=Jtr, col=(keys % N).astype(np.int32),
                row_ptr=np.searchsorted(rows, np.arange(N + 1)).astype(np.int32))


def ring_rows(rng, members, rows_per_node=ROWS_PER_NODE):
    """rows_per_node rows per member a, each touching members[(a + OFFSETS) mod len] (nodes may repeat in a short ring)."""
    members = np.asarray(members, dtype=np.int64)
    base = np.repeat(np.arange(len(members)), rows_per_node)
    nodes = members[(base[:, None] + np.array(OFFSETS)[None, :]) % len(members)]
    return nodes, rng.standard_normal((len(base), len(OFFSETS), 6)), rng.standard_normal(len(base))


def edge_rows(rng, edges, per_edge=3):
    nodes = np.repeat(np.asarray(edges, dtype=np.int64).reshape(-1, 2), per_edge, axis=0)
    return nodes, rng.standard_normal((len(nodes), 2, 6)), rng.standard_normal(len(nodes))


def unary_rows(rng, node, count=8):
    return np.full((count, 1), node, dtype=np.int64), rng.standard_normal((count, 1, 6)), rng.standard_normal(count)


def widths(sys):
    return np.diff(sys["row_ptr"])


def diagonal_position(sys, a):
    """Position of row a's diagonal block within the row (the persistent kernel caches positions 0 .. ROW_CACHE - 1)."""
    beg, end = sys["row_ptr"][a], sys["row_ptr"][a + 1]
    pos = np.flatnonzero(sys["col"][beg:end] == a)
    assert len(pos) == 1
    return int(pos[0])


def _case(name, family, sys, lm=LM, claims=(), compare_converged=True, **extra):
    return dict(sys, name=name, family=family, lm=lm, claims=tuple(claims), compare_converged=compare_converged, **extra)


@functools.lru_cache(maxsize=None)
def standard(N, seed=0):
    rng = np.random.default_rng(1000 + 7 * N + seed)
    return gram_system(N, [ring_rows(rng, np.arange(N))])


@functools.lru_cache(maxsize=None)
def widths_system():
    """N = 64.  Node 0 isolated (a row of its diagonal alone); node 1 a hub of nodes 2..63 (63 blocks); nodes 2, 3, 4, 5 with
    exactly 31, 30, 11, 10 blocks; a ring over 6..63."""
    rng = np.random.default_rng(64001)
    edges = [(1, b) for b in range(2, 64)]
    edges += [(2, b) for b in range(6, 35)] + [(3, b) for b in range(6, 34)]
    edges += [(4, b) for b in range(35, 44)] + [(5, b) for b in range(35, 43)]
    return gram_system(64, [ring_rows(rng, np.arange(6, 64)), edge_rows(rng, edges), unary_rows(rng, 0)])


WIDTH_CLAIMS = {0: 1, 5: 10, 4: 11, 3: 30, 2: 31, 1: 63}           # node -> blocks in its row


@functools.lru_cache(maxsize=None)
def late_diagonal_system():
    """N = 64.  Node 63 is a hub of all others (diagonal at position 63 of its row); node 40 is connected to 0..34 and the hub
    (diagonal at position 35): both beyond the ROW_CACHE blocks the persistent kernel holds in registers."""
    rng = np.random.default_rng(64002)
    ring = [a for a in range(63) if a != 40]
    edges = [(63, b) for b in range(63)] + [(40, b) for b in range(35)]
    return gram_system(64, [ring_rows(rng, ring), edge_rows(rng, edges)])


LATE_DIAGONALS = {63: 63, 40: 35}                                   # node -> position of its diagonal block


@functools.lru_cache(maxsize=None)
def starved_system():
    """N = 41.  Nodes 38 and 39 are touched by no row (zero diagonal block, zero rhs); node 40 by ONE row (a rank-1 diagonal
    block), whose piece at node 40 is dyadic with a leading 1/4: its Cholesky is exact and pivots 2..6 are exactly 0, so the
    kernel's pivot rule decides them (and not the last bit of a rounded difference).  Jacobian entries of 0.1 standard
    deviation: with LM_WEAK's lm_abs = 1e-3 on the empty nodes' diagonals the condition number stays below 1e4."""
    rng = np.random.default_rng(41001)
    nodes, J, r = ring_rows(rng, np.arange(38))
    Js = 0.1 * rng.standard_normal((1, 4, 6))
    Js[0, 0] = [0.25, 0.5, -0.25, 0.125, -0.5, 0.375]
    single = (np.array([[40, 0, 1, 2]]), Js, np.array([0.75]))
    return gram_system(41, [(nodes, 0.1 * J, r), single])


STARVED_EMPTY, STARVED_RANK1 = (38, 39), 40


def _zero_rhs(partial):
    sys = dict(standard(41, seed=3))
    Jtr = sys["Jtr"].copy()
    if partial:
        Jtr[ZERO_RHS_ROWS] = 0.0
    else:
        Jtr[:] = 0.0
    sys["Jtr"] = Jtr
    return sys


ZERO_RHS_ROWS = np.array([0, 3, 7, 8, 9, 20, 21, 33, 39, 40])


# (kept as a constant so that collecting the tests builds no system; test_pcg_cases.py holds it against cases())
NAMES = ("tiny-1", "tiny-2", "tiny-8", "tiny-9", "tiny-10", "tiny-11", "groups-40", "groups-41", "groups-256", "groups-257",
         "wg64-512", "wg64-513", "widths", "late_diagonal", "starved-undamped", "starved-damped", "zero_rhs-all",
         "zero_rhs-ten_rows", "big16", "beyond")
CONVERGED_NAMES = ("groups-40", "groups-41", "groups-256", "groups-257", "wg64-512", "wg64-513", "widths", "late_diagonal",
                   "zero_rhs-ten_rows", "big16", "beyond")
SMALL_NAMES = NAMES[:10] + NAMES[12:18]                                # N <= 300: a dense eigen-decomposition is cheap


def shape_sizes(n_cu=256):
    """N of the two cases that depend on the device: the first automatic 16-wave persistent grid, and a grid beyond the
    persistent kernel (more than 16 n_cu rows: the automatic multi-launch path)."""
    return 8 * n_cu + 2, 16 * n_cu + 4


def cases(n_cu=256):
    """Every named case as a dict: the system (N, keys, blocks, Jtr, row_ptr, col), name, family, lm, claims."""
    out = []
    for N in (1, 2, 8, 9, 10, 11):
        out.append(_case("tiny-%d" % N, "tiny", standard(N), compare_converged=False))
    for N in (40, 41, 256, 257):
        out.append(_case("groups-%d" % N, "groups", standard(N)))
    for N in (512, 513):
        out.append(_case("wg64-%d" % N, "wg64", standard(N), claims=("wg64",)))
    out.append(_case("widths", "widths", widths_system(), claims=("widths",)))
    out.append(_case("late_diagonal", "late_diagonal", late_diagonal_system(), claims=("late_diagonal",)))
    out.append(_case("starved-undamped", "starved", starved_system(), lm=(0.0, 0.0), claims=("starved", "singular"),
                     compare_converged=False))
    out.append(_case("starved-damped", "starved", starved_system(), lm=LM_WEAK, claims=("starved",), compare_converged=False))
    out.append(_case("zero_rhs-all", "zero_rhs", _zero_rhs(False), claims=("zero_rhs",), compare_converged=False))
    out.append(_case("zero_rhs-ten_rows", "zero_rhs", _zero_rhs(True), claims=("zero_rhs_partial",)))
    n16, nbeyond = shape_sizes(n_cu)
    out.append(_case("big16", "big16", standard(n16), claims=("big16",)))
    out.append(_case("beyond", "beyond", standard(nbeyond), claims=("beyond",)))
    return out


def case(name, n_cu=256):
    return next(c for c in cases(n_cu) if c["name"] == name)


def workgroups(N, wpb):
    """Workgroups of the persistent kernel: one wave per row, wpb waves per workgroup."""
    return (N + wpb - 1) // wpb


def auto_wpb(N, n_cu):
    """pcg_shape's choice (csrc/dfh_pcg.hip): 8 waves while the grid fits one workgroup per CU, 16 beyond."""
    return 8 if (N + 7) // 8 <= n_cu else 16


def dense(c, damped=True):
    """The case's matrix as a dense array, with its damping (what the oracles solve)."""
    from oracle import gn_np as G
    blocks = G.damp_blocks(c["N"], c["keys"], c["blocks"], *c["lm"]) if damped else c["blocks"]
    return G.blocks_to_bsr(c["N"], c["keys"], blocks).toarray()
