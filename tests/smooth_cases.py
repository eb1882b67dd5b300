"""The small meshes K25's tests run on (tests/test_smooth_np.py on the CPU, tests/test_gpu_smooth.py on the device): each the
smallest at which one thing can go wrong.  CASES[name] = (verts (V, 3) float64, faces (F, 3) int32); FLAGGED[name] = how many
vertices the boundary rule flags.  simplify_cases.sphere and cube are NOT closed (duplicate pole and seam vertices): they are
used as open cases only."""
import numpy as np

from simplify_cases import grid_faces, lattice, sphere

CENTRE = (12.3, 12.1, 11.7)
RADIUS = 10.0


def icosphere(level, r=RADIUS, centre=CENTRE):
    """A properly welded icosphere: 10 * 4^level + 2 vertices, 20 * 4^level faces, closed, outward winding."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.sqrt(1.0 + t * t) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.sqrt((m * m).sum()))
                mid[key] = len(v) - 1
            return mid[key]
        g = []
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.asarray(v) * r + np.asarray(centre), np.asarray(f, dtype=np.int32)


def noisy_icosphere(level=3, seed=7, sigma=0.1):
    """The recovery scene: icosphere(level) with radial noise default_rng(seed).normal(0, sigma, (V, 1))."""
    v, f = icosphere(level)
    d = v - np.asarray(CENTRE)
    r = np.sqrt((d * d).sum(axis=1, keepdims=True))
    noise = np.random.default_rng(seed).normal(0.0, sigma, (len(v), 1))
    return np.asarray(CENTRE) + d / r * (r + noise), f


def bipyramid(rim=300):
    """A closed fan: `rim` vertices on a wavy circle, a lower hub, and an upper hub of valence `rim` with the highest index."""
    a = 2.0 * np.pi * np.arange(rim) / rim
    v = np.concatenate([np.stack([10.0 * np.cos(a), 10.0 * np.sin(a), 0.3 * np.sin(3 * a)], axis=1), [[0.1, -0.2, -3.0], [0.2, 0.1, 2.0]]])
    i = np.arange(rim)
    j = (i + 1) % rim
    f = np.concatenate([np.stack([np.full(rim, rim + 1), i, j], axis=1), np.stack([np.full(rim, rim), j, i], axis=1)])
    return v, f.astype(np.int32)


def wavy(nu, nv):
    return lattice(nu, nv, lambda i, j: 0.3 * np.sin(1.3 * i + 0.7 * j))


def _cases():
    c, n = {}, {}
    none = np.zeros((0, 3), dtype=np.int32)
    c["empty"], n["empty"] = (np.zeros((0, 3)), none), 0
    c["no_faces"], n["no_faces"] = (np.array([[0.1, 0.2, 0.3], [0.4, 0.1, 0.2], [3.0, 0.0, 0.0], [3.2, 0.1, 0.4]]), none), 0
    c["triangle"], n["triangle"] = (np.array([[0.1, 0.1, 0.1], [1.6, 0.2, 0.1], [0.2, 1.7, 0.3]]), np.array([[0, 1, 2]], dtype=np.int32)), 3
    tet = np.array([[0.1, 0.2, 0.3], [1.3, 0.1, 0.2], [0.4, 1.2, 0.1], [0.5, 0.4, 1.1]])
    tet_f = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int32)
    c["tetrahedron"], n["tetrahedron"] = (tet, tet_f), 0
    c["icosphere_1"], n["icosphere_1"] = icosphere(1), 0
    c["icosphere_3"], n["icosphere_3"] = icosphere(3), 0
    c["lattice_9x7"], n["lattice_9x7"] = wavy(9, 7), 28                     # open: the rim is flagged
    c["lattice_33x33"], n["lattice_33x33"] = wavy(33, 33), 128               # 1 089 vertices: more than one workgroup of 256 and 1 024
    c["bipyramid_hub_last"], n["bipyramid_hub_last"] = bipyramid(), 0
    # three triangles on the edge (0, 1): its two ends see the other end three times; the three tips lie on open edges
    c["three_on_one_edge"] = (np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.2], [0.4, 1.0, 0.1], [0.5, -0.9, 0.3], [0.6, 0.1, 1.2]]),
                              np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int32))
    n["three_on_one_edge"] = 5
    # a face listed twice on a closed mesh: its three corners see each other four times
    c["face_twice"], n["face_twice"] = (tet * 1.7, np.concatenate([tet_f, tet_f[1:2]]).astype(np.int32)), 3
    lv, lf = wavy(6, 6)
    # a face with two equal corners, (14, 14, 20): vertex 14 has two entries that name itself, and 14 and its neighbour 20
    # see each other four times (both interior, both flagged)
    c["face_names_vertex_twice"] = (lv, np.concatenate([lf[:7], [[14, 14, 20]], lf[7:]]).astype(np.int32))
    n["face_names_vertex_twice"] = 22
    cv = lv.copy()
    cv[15] = cv[14]                                                          # coincident vertices: zero-area faces, zero cotangent weights
    c["coincident_vertices"], n["coincident_vertices"] = (cv, lf), 20
    # an obtuse face on a closed mesh: a flat tetrahedron whose apex lies close above the base's longest edge
    c["obtuse"] = (np.array([[0.0, 0.0, 0.0], [4.0, 0.0, 0.1], [2.0, 3.0, 0.0], [2.1, 0.2, 0.3]]), tet_f)
    n["obtuse"] = 0
    extra = np.array([[0.2, 0.3, 0.05], [40.0, 40.0, 40.0], [2.6, 2.2, 0.2]])
    c["isolated_vertices"], n["isolated_vertices"] = (np.concatenate([extra[:2], lv, extra[2:]]), lf + 2), 20
    c["sphere_open_seams"], n["sphere_open_seams"] = sphere(nlat=6, nlon=8), None          # duplicate pole vertices: an open case
    return c, n


CASES, FLAGGED = _cases()
CLOSED = ["tetrahedron", "icosphere_1", "icosphere_3", "bipyramid_hub_last", "obtuse"]
