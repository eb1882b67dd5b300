"""The meshes of the K23 tests (connected components): small, built here, every one at a shape where labelling, the table or the
compaction can go wrong.  CASES: name -> (verts (V, 3) float64, faces (F, 3) int32)."""
import numpy as np


def _verts(n, seed):
    """n points with coordinates that are not round numbers (so that area sums really depend on their order)."""
    return np.random.default_rng(seed).uniform(-3.0, 3.0, size=(n, 3))


def _faces(rows):
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3)


def strip(n_faces, relabel=None):
    """A triangle strip: face i = (i, i + 1, i + 2), the vertex ids passed through `relabel`."""
    i = np.arange(n_faces)
    f = np.stack([i, i + 1, i + 2], axis=1)
    return _faces(f if relabel is None else relabel[f])


def fan(n_faces):
    """n faces round one hub vertex whose index is the highest."""
    i = np.arange(n_faces)
    return _faces(np.stack([np.full(n_faces, n_faces + 1), i, i + 1], axis=1))


def isolated(n_tri):
    return _faces(np.arange(3 * n_tri).reshape(-1, 3))


def soup(V, F, seed):
    """F faces over V vertices in short runs: several components of mixed size, some vertices unreferenced."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, max(V - 2, 1), size=F)
    return _faces(np.stack([base, np.minimum(base + rng.integers(0, 3, size=F), V - 1), np.minimum(base + 2, V - 1)], axis=1))


def _cases():
    c = {}
    c["no_vertices"] = (np.zeros((0, 3)), _faces([]))
    c["no_faces_5_verts"] = (_verts(5, 1), _faces([]))
    c["one_face"] = (_verts(3, 2), _faces([[0, 1, 2]]))
    c["two_faces_sharing_a_vertex"] = (_verts(5, 3), _faces([[0, 1, 2], [2, 3, 4]]))
    c["two_disjoint_faces"] = (_verts(6, 4), _faces([[3, 4, 5], [0, 1, 2]]))
    n = 20000
    c["strip_reversed"] = (_verts(n + 2, 5), strip(n, np.arange(n + 2)[::-1]))
    c["strip_permuted"] = (_verts(n + 2, 6), strip(n, np.random.default_rng(7).permutation(n + 2)))
    c["fan_hub_last"] = (_verts(5002, 8), fan(5000))
    c["isolated_3000"] = (_verts(9000, 9), isolated(3000))
    # one table entry per face, and cc_table_rank_kernel strides 2048 workgroups x 4 waves over the entries: at 8193 the first wave
    # takes a second entry
    c["isolated_8193"] = (_verts(3 * 8193, 60), isolated(8193))
    for k in (255, 256, 257, 1023, 1024, 1025):
        c["soup_%d" % k] = (_verts(k, 10 + k), soup(k, k, 20 + k))              # V = F = k
        c["strip_F%d" % k] = (_verts(k + 2, 30 + k), strip(k))                  # F = k, one component
        c["isolated_V%d" % k] = (_verts(k, 40 + k), isolated(k // 3))           # V = k, k % 3 unreferenced at the end
    # degenerate faces (a == b, a == b == c), duplicates, unreferenced vertices in front (0, 1), in the middle (6) and at the end (11)
    c["degenerate_duplicate_unreferenced"] = (_verts(12, 50), _faces([[2, 2, 3], [3, 4, 5], [3, 4, 5], [5, 5, 5], [7, 8, 8], [9, 10, 9],
                                                                      [8, 9, 7], [4, 2, 2]]))
    return c


CASES = _cases()
KEEP_MASKS = ("all", "none", "alternating", "last")


def keep_mask(kind, n):
    k = np.zeros(n, dtype=np.uint8)
    if kind == "all":
        k[:] = 1
    elif kind == "alternating":
        k[::2] = 1
    elif kind == "last" and n:
        k[-1] = 1
    return k
