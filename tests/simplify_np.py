"""The numpy restatement of K24 (mesh simplification by vertex clustering with quadrics), operation by operation as
include/dfusion_hip.h defines it: fp64, one rounding per operation (every line below is one elementwise numpy operation per
arithmetic operation: no cross, einsum, matmul or linalg, which may fuse or reorder), sums from 0.0 in the stated order
(np.add.at adds unbuffered, in the order of its index array).  The device must equal it bit for bit."""
import numpy as np

LIMIT = 1 << 21


def cells(verts, cell, origin):
    """(c (V, 3) int64, key (V,) int64, ctr (V, 3) float64); ValueError for what the device refuses."""
    p = np.asarray(verts).astype(np.float64)
    if not np.isfinite(p).all():
        raise ValueError("a vertex coordinate is not finite")
    o = np.asarray(origin, dtype=np.float64)
    q = np.floor((p - o) / np.float64(cell))
    if not ((q >= 0) & (q < LIMIT)).all():
        raise ValueError("a vertex lies outside the 2^21 cells an axis")
    c = q.astype(np.int64)
    key = (c[:, 0] << 42) + (c[:, 1] << 21) + c[:, 2]
    ctr = o + (q + 0.5) * np.float64(cell)
    return c, key, ctr


def cluster_ids(key):
    """(vert_cluster (V,) int64, C): ids in ascending order of the cluster's lowest vertex index."""
    if len(key) == 0:
        return np.zeros(0, dtype=np.int64), 0
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    ident = np.empty(len(first), dtype=np.int64)
    ident[np.argsort(first, kind="stable")] = np.arange(len(first))
    return ident[inverse.reshape(-1)], len(first)


def vertex_quadrics(p, faces, ctr):
    """Q_v (V, 10): over the (face, corner) entries that name v, ascending face then corner."""
    V = len(p)
    Q = np.zeros((V, 10))
    if len(faces) == 0:
        return Q
    a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
    e1, e2 = b - a, c - a
    n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    ent = faces.reshape(-1)                                  # entry e = 3 f + corner names vertex ent[e]
    rep = lambda x: np.repeat(x, 3, axis=0)
    N0, N1, N2 = rep(n0), rep(n1), rep(n2)
    q = rep(a) - ctr[ent]
    d = -((N0 * q[:, 0] + N1 * q[:, 1]) + N2 * q[:, 2])
    ten = np.stack([N0 * N0, N0 * N1, N0 * N2, N1 * N1, N1 * N2, N2 * N2, d * N0, d * N1, d * N2, d * d], axis=1)
    np.add.at(Q, ent, ten)
    return Q


def representatives(m, QC, cell, mode, reg):
    """(x (C, 3), fell (C,) bool): the LDL^T solve of the header, in its order; a failed test keeps the mean."""
    if mode == "mean":
        return m.copy(), np.zeros(len(m), dtype=bool)
    A00, A01, A02, A11, A12, A22, b0, b1, b2 = (QC[:, k] for k in range(9))
    with np.errstate(all="ignore"):
        t = (A00 + A11) + A22
        lam = np.float64(reg) * t
        M00, M10, M20, M11, M21, M22 = A00 + lam, A01, A02, A11 + lam, A12, A22 + lam
        r0, r1, r2 = lam * m[:, 0] - b0, lam * m[:, 1] - b1, lam * m[:, 2] - b2
        d0 = M00
        l10, l20 = M10 / d0, M20 / d0
        d1 = M11 - l10 * M10
        t21 = M21 - l20 * M10
        l21 = t21 / d1
        d2 = (M22 - l20 * M20) - l21 * t21
        y0 = r0
        y1 = r1 - l10 * y0
        y2 = (r2 - l20 * y0) - l21 * y1
        x2 = y2 / d2
        x1 = y1 / d1 - l21 * x2
        x0 = (y0 / d0 - l10 * x1) - l20 * x2
        half = 0.5 * np.float64(cell)
        ok = (t > 0) & (d0 > 0) & (d1 > 0) & (d2 > 0) & (np.abs(x0) <= half) & (np.abs(x1) <= half) & (np.abs(x2) <= half)
    x = np.where(ok[:, None], np.stack([x0, x1, x2], axis=1), m)
    return x, ~ok


def simplify(verts, faces, attrs=(), *, cell, origin=None, mode="quadric", reg=1e-3, drop_unreferenced=True):
    """-> dict(verts, faces, attrs, vert_map, face_idx, n_clusters, n_fallback, vert_cluster, cluster_verts): the mesh after
    the drop, cluster_verts the (C, 3) positions before it.  n_clusters and n_fallback count the clusters before the drop."""
    if mode not in ("quadric", "mean"):
        raise ValueError("mode")
    verts = np.asarray(verts)
    dtype = verts.dtype
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    V, F = len(verts), len(faces)
    if F and (faces.min() < 0 or faces.max() >= V):
        raise ValueError("a face holds a vertex index outside [0, V)")
    p = verts.astype(np.float64).reshape(-1, 3)
    if origin is None:
        origin = p.min(axis=0) if V else np.zeros(3)
    _, key, ctr = cells(p, cell, origin)
    vc, C = cluster_ids(key)

    count = np.zeros(C, dtype=np.int64)
    np.add.at(count, vc, 1)
    S = np.zeros((C, 3))
    np.add.at(S, vc, p - ctr)
    m = S / count.astype(np.float64)[:, None]
    cctr = np.zeros((C, 3))
    cctr[vc] = ctr                                           # (the same centre for every member)
    QC = np.zeros((C, 10))
    if mode == "quadric":
        np.add.at(QC, vc, vertex_quadrics(p, faces, ctr))
    x, fell = representatives(m, QC, cell, mode, reg)
    cluster_verts = (cctr + x).astype(dtype)

    out_attrs = []
    for a in attrs:
        a = np.asarray(a)
        s = np.zeros((C,) + a.shape[1:])
        np.add.at(s, vc, a.astype(np.float64))
        out_attrs.append((s / count.astype(np.float64).reshape((C,) + (1,) * (a.ndim - 1))).astype(a.dtype))

    cf = vc[faces] if F else np.zeros((0, 3), dtype=np.int64)
    alive = np.nonzero((cf[:, 0] != cf[:, 1]) & (cf[:, 1] != cf[:, 2]) & (cf[:, 0] != cf[:, 2]))[0]
    if len(alive):
        _, first = np.unique(np.sort(cf[alive], axis=1), axis=0, return_index=True)
        face_idx = np.sort(alive[first])
    else:
        face_idx = np.zeros(0, dtype=np.int64)
    new_faces = cf[face_idx]
    if drop_unreferenced:
        kept = np.unique(new_faces)
    else:
        kept = np.arange(C)
    cmap = np.full(C, -1, dtype=np.int64)
    cmap[kept] = np.arange(len(kept))
    return dict(verts=cluster_verts[kept], faces=cmap[new_faces].astype(np.int32).reshape(-1, 3), attrs=[a[kept] for a in out_attrs],
                vert_map=cmap[vc] if V else np.zeros(0, dtype=np.int64), face_idx=face_idx, n_clusters=C, n_fallback=int(fell.sum()),
                vert_cluster=vc, cluster_verts=cluster_verts)


# ---- what the golden records (tools/make_simplify_golden.py writes it, tests/test_simplify_np.py reproduces it) ---------------
def box_surface_distance(p, lo, hi):
    """|distance| of points to the surface of the axis-aligned box [lo, hi]^3."""
    p = np.asarray(p, dtype=np.float64)
    out = np.maximum(np.maximum(lo - p, p - hi), 0.0)
    outside = np.sqrt((out * out).sum(axis=1))
    inside = np.minimum(p - lo, hi - p).min(axis=1)
    return np.where(outside > 0, outside, np.abs(inside))


def cube_measures(verts, side, offset):
    p = np.asarray(verts, dtype=np.float64)
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64) * side + offset
    near = np.sqrt(((corners[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)).min(axis=1)
    d = box_surface_distance(p, offset, offset + side)
    return {"corner_distance_max": float(near.max()), "surface_error_mean": float(d.mean()), "surface_error_max": float(d.max())}


def sphere_measures(verts, centre, r):
    p = np.asarray(verts, dtype=np.float64) - np.asarray(centre, dtype=np.float64)
    e = np.sqrt((p * p).sum(axis=1)) - r
    return {"radial_error_signed_mean": float(e.mean()), "radial_error_abs_mean": float(np.abs(e).mean()), "radial_error_abs_max": float(np.abs(e).max())}


def golden_record(cases, reg_cases, cube_geometry, sphere_case):
    """Counts of every case in both modes (reg 1e-3, and reg 0 on reg_cases), the cube's and the sphere's measures."""
    rec = {"counts": {}, "cube": {}, "sphere": {}}
    for name in sorted(cases):
        v, f, cell, origin = cases[name]
        for mode in ("quadric", "mean"):
            for reg in ([1e-3, 0.0] if (name in reg_cases and mode == "quadric") else [1e-3]):
                r = simplify(v, f, cell=cell, origin=origin, mode=mode, reg=reg)
                rec["counts"]["%s/%s/reg=%g" % (name, mode, reg)] = {"verts": int(len(r["verts"])), "faces": int(len(r["faces"])),
                                                                    "clusters": int(r["n_clusters"]), "fallback": int(r["n_fallback"])}
    v, f, cell, origin = cases["cube"]
    (sv, sf, scell, centre, radius) = sphere_case
    for mode in ("quadric", "mean"):
        rec["cube"][mode] = cube_measures(simplify(v, f, cell=cell, origin=origin, mode=mode)["verts"], *cube_geometry)
        rec["sphere"][mode] = sphere_measures(simplify(sv, sf, cell=scell, mode=mode)["verts"], centre, radius)
    return rec
