"""The small meshes K24's tests run on (tests/test_simplify_np.py on the CPU, tests/test_gpu_simplify.py on the device): each the
smallest at which one thing can go wrong.  CASES[name] = (verts (V, 3) float64, faces (F, 3) int32, cell, origin or None)."""
import numpy as np


def grid_faces(nu, nv, base=0, flip=False):
    """Two triangles a quad of an nu x nv lattice whose vertex (i, j) has index base + i * nv + j."""
    i, j = np.meshgrid(np.arange(nu - 1), np.arange(nv - 1), indexing="ij")
    a = (base + i * nv + j).reshape(-1)
    b, c, d = a + nv, a + nv + 1, a + 1
    f = np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)])
    return (f[:, ::-1] if flip else f).astype(np.int32)


def lattice(nu, nv, height):
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    v = np.stack([i, j, height(i, j)], axis=-1).reshape(-1, 3).astype(np.float64)
    return v, grid_faces(nu, nv)


def cube(n=17, offset=0.25):
    """Six faces of n x n lattice vertices, spacing 1, from `offset` to `offset + n - 1`: ranks 1 (faces), 2 (edges), 3 (corners)."""
    t = np.arange(n, dtype=np.float64)
    u, w = np.meshgrid(t, t, indexing="ij")
    lo, hi = np.zeros_like(u), np.full_like(u, n - 1.0)
    sides = [(lo, u, w), (hi, u, w), (u, lo, w), (u, hi, w), (u, w, lo), (u, w, hi)]
    verts, faces = [], []
    for s, xyz in enumerate(sides):
        verts.append(np.stack(xyz, axis=-1).reshape(-1, 3) + offset)
        faces.append(grid_faces(n, n, base=s * n * n, flip=s % 2 == 1))
    return np.concatenate(verts), np.concatenate(faces)


def cube_side():
    return 16.0, 0.25                                        # edge length and offset of cube()


def sphere(r=10.0, nlat=40, nlon=80, centre=(12.3, 12.1, 11.7)):
    th = np.pi * (np.arange(nlat + 1) / nlat)
    ph = 2.0 * np.pi * (np.arange(nlon) / nlon)
    T, P = np.meshgrid(th, ph, indexing="ij")
    v = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], axis=-1).reshape(-1, 3) * r + np.asarray(centre)
    f = []
    for i in range(nlat):
        for j in range(nlon):
            a, b = i * nlon + j, i * nlon + (j + 1) % nlon
            f += [(a, a + nlon, b + nlon), (a, b + nlon, b)]
    return v, np.asarray(f, dtype=np.int32)


def strip(nv):
    """nv vertices in a zigzag, nv - 2 faces; at cell 0.5 every vertex has a cell of its own."""
    i = np.arange(nv)
    v = np.stack([i * 1.0, (i % 2) * 1.0, 0.25 * (i % 3)], axis=1)
    f = np.stack([i[:-2], i[:-2] + 1, i[:-2] + 2], axis=1).astype(np.int32)
    return v, f


def fan_hub_last(rim=1100):
    a = 2.0 * np.pi * np.arange(rim) / rim
    v = np.concatenate([np.stack([10.0 * np.cos(a), 10.0 * np.sin(a), 0.3 * np.sin(3 * a)], axis=1), [[0.2, 0.1, 2.0]]])
    i = np.arange(rim)
    f = np.stack([np.full(rim, rim), i, (i + 1) % rim], axis=1).astype(np.int32)
    return v, f


def crowded_cell(n=1200, seed=5):
    rng = np.random.default_rng(seed)
    inside = rng.uniform(0.0, 1.0, (n, 3))
    ring = np.stack([np.cos(np.arange(12.0)), np.sin(np.arange(12.0)), 0.1 * np.arange(12.0)], axis=1) * 4.0 + 0.5
    v = np.concatenate([inside, ring])
    f = np.concatenate([rng.integers(0, n, (900, 3)), np.stack([rng.integers(0, n, 300), n + rng.integers(0, 12, 300), n + rng.integers(0, 12, 300)], axis=1)])
    return v, f.astype(np.int32)


def permuted(v, f, seed=3):
    perm = np.random.default_rng(seed).permutation(len(v))   # new index i holds old vertex perm[i]
    inv = np.empty(len(v), dtype=np.int64)
    inv[perm] = np.arange(len(v))
    return v[perm], inv[f].astype(np.int32), perm


def _cases():
    c = {}
    none = np.zeros((0, 3), dtype=np.int32)
    c["empty"] = (np.zeros((0, 3)), none, 1.0, None)
    c["no_faces"] = (np.array([[0.1, 0.2, 0.3], [0.4, 0.1, 0.2], [3.0, 0.0, 0.0], [3.2, 0.1, 0.4]]), none, 1.0, None)
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    c["triangle_one_cell"] = (np.array([[0.1, 0.1, 0.1], [0.6, 0.2, 0.1], [0.2, 0.7, 0.3]]), tri, 1.0, (0.0, 0.0, 0.0))
    c["triangle_three_cells"] = (np.array([[0.1, 0.1, 0.1], [1.6, 0.2, 0.1], [0.2, 1.7, 0.3]]), tri, 1.0, (0.0, 0.0, 0.0))
    lv, lf = lattice(9, 8, lambda i, j: (i * j) % 3)
    c["lattice_cell1"] = (lv, lf, 1.0, None)                 # integer coordinates, integer origin: every vertex on a cell boundary
    c["lattice_cell2"] = (lv, lf, 2.0, None)
    pv, pf = lattice(12, 12, lambda i, j: 0.0 * i)
    c["plane"] = (pv * 0.7 + np.array([0.0, 0.0, 0.3]), pf, 2.0, (-0.1, -0.1, -0.1))
    tv, tf = lattice(12, 11, lambda i, j: 0.25 * i + 0.5 * j)
    c["plane_tilted"] = (tv * 0.7, tf, 2.0, None)
    cv, cf = cube()
    c["cube"] = (cv, cf, 3.0, None)
    sv, sf = lattice(10, 9, lambda i, j: 0.0 * i)
    top = sv * 0.8 + np.array([0.1, 0.1, 0.3])
    c["thin_sheet"] = (np.concatenate([top, top - np.array([0.0, 0.0, 0.2])]), np.concatenate([sf, grid_faces(10, 9, base=90, flip=True)]), 1.5,
                       (0.0, 0.0, 0.0))
    fv, ff = fan_hub_last()
    c["fan_hub_last"] = (fv, ff, 1.0, None)
    wv, wf = crowded_cell()
    c["crowded_cell"] = (wv, wf, 1.0, (-4.0, -4.0, -4.0))    # the cell [0, 1)^3 holds 1 200 vertices
    iv, if_ = lattice(6, 6, lambda i, j: 0.1 * i)
    extra = np.array([[0.2, 0.3, 0.05], [40.0, 40.0, 40.0], [2.6, 2.2, 0.2], [40.3, 40.2, 40.1], [-3.0, 2.0, 1.0]])
    c["isolated_unreferenced"] = (np.concatenate([extra[:2], iv, extra[2:]]), if_ + 2, 1.5, None)
    c["face_names_vertex_twice"] = (iv, np.concatenate([if_[:7], [[3, 3, 20], [8, 14, 8]], if_[7:]]).astype(np.int32), 1.5, None)
    dv, df = strip(40)
    dup = np.concatenate([df[:10], df[3:6], df[4:5, ::-1], df[7:8, [1, 2, 0]], df[10:], df[20:22], [[5, 5, 6]]]).astype(np.int32)
    c["duplicate_faces"] = (dv, dup, 0.5, None)
    for n in (1023, 1024, 1025, 1026, 1027):                 # V = C = n, F = n - 2: the scan's block edges, one vertex a cell
        v, f = strip(n)
        c["strip_%d" % n] = (v, f, 0.5, None)
    v, f = lattice(80, 40, lambda i, j: 0.3 * ((i * j) % 3))  # clustered: V, F, C and F' each cross chunk edges of their own
    c["lattice_80x40_cell1.5"] = (v, f, 1.5, None)
    qv, qf, _ = permuted(cv, cf)
    c["cube_permuted"] = (qv, qf, 3.0, None)
    return c


CASES = _cases()
ONE_VERTEX_A_CELL = ["duplicate_faces"] + ["strip_%d" % n for n in (1023, 1024, 1025, 1026, 1027)]
REG_CASES = ["cube", "plane", "plane_tilted"]
