"""Meshes and analytic answers shared by the K22 tests (tests/test_mesh_sdf_np.py on the CPU, tests/test_gpu_mesh_sdf.py)."""
import numpy as np

L_POLY = np.array([(0, 0), (4, 0), (4, 2), (2, 2), (2, 4), (0, 4)], dtype=np.float64)
L_HEIGHT = 3.0


def l_prism():
    """The closed L-shaped prism: L_POLY (counter-clockwise) extruded to z in [0, 3]; 12 vertices, 20 faces wound outward."""
    n = len(L_POLY)
    v = np.concatenate([np.c_[L_POLY, np.zeros(n)], np.c_[L_POLY, np.full(n, L_HEIGHT)]])
    cap = [(0, 1, 2), (0, 2, 3), (0, 3, 5), (3, 4, 5)]            # a triangulation of the L
    f = [(a, c, b) for a, b, c in cap]                             # bottom: facing -z
    f += [(a + n, b + n, c + n) for a, b, c in cap]                # top: facing +z
    for i in range(n):
        j = (i + 1) % n
        f += [(i, j, j + n), (i, j + n, i + n)]
    return v, np.array(f, dtype=np.int32)


def l_inside(P):
    """Strictly inside the L prism (the tests' grids have no vertex on its surface)."""
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    in_l = (x > 0) & (y > 0) & (((x < 4) & (y < 2)) | ((x < 2) & (y < 4)))
    return in_l & (z > 0) & (z < L_HEIGHT)


L_GRID = dict(origin=-2.25, spacing=0.5, shape=(18, 18, 18))


def cube(lo=0.0, hi=4.0):
    """An axis-aligned cube on lattice vertices, 12 faces wound outward."""
    c = np.array([(x, y, z) for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], dtype=np.float64)
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
    return c, np.array(f, dtype=np.int32)


def box_distance(P, lo, hi):
    """Distance from points OUTSIDE or on the box [lo, hi]^3 to it."""
    g = np.maximum(np.maximum(lo - P, P - hi), 0.0)
    return np.sqrt((g * g).sum(-1))


def icosphere(level, radius=1.0, center=0.0):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius + center, np.array(f, dtype=np.int32)


def soup(n_faces, seed, scale=8.0, size=1.5):
    """n_faces random small triangles in [0, scale]^3, no shared vertices."""
    r = np.random.RandomState(seed)
    c = r.uniform(0, scale, (n_faces, 1, 3))
    v = (c + r.uniform(-size, size, (n_faces, 3, 3))).reshape(-1, 3)
    return v, np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)


def fan(n_faces, seed=5):
    """n_faces thin triangles around one shared vertex: all of them land in the apex's cell."""
    r = np.random.RandomState(seed)
    rim = r.normal(size=(n_faces + 1, 3))
    rim = 0.5 * rim / np.linalg.norm(rim, axis=1, keepdims=True)
    v = np.concatenate([[[3.0, 3.0, 3.0]], 3.0 + rim])
    return v, np.array([(0, 1 + i, 2 + i) for i in range(n_faces)], dtype=np.int32)


def big_and_tiny(seed=9):
    """One face spanning the whole table beside 40 tiny ones."""
    v, f = soup(40, seed, scale=8.0, size=0.2)
    big = np.array([[-1.0, -1.0, 4.0], [9.0, -1.0, 4.5], [4.0, 9.0, 3.5]])
    return np.concatenate([v, big]), np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)
