"""The K22 result (include/dfusion_hip.h, "mesh -> signed distance") restated in numpy: brute force over ALL faces with the
header's operations, the far fill, and a slow, loop-written version of the pseudonormal tables.  No search structure: the result
is a minimum over a set, so this is what any search must reproduce bit for bit."""
import math

import numpy as np


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def widen(verts, faces):
    return np.ascontiguousarray(np.asarray(verts), dtype=np.float64), np.ascontiguousarray(np.asarray(faces), dtype=np.int64)


def pseudonormals_loops(verts, faces):
    """(face_normals, edge_normals, vertex_normals, dropped), written with loops over faces, edges and corners."""
    v, f = widen(verts, faces)
    F = len(f)
    fn = np.zeros((F, 3))
    en = np.zeros((F, 3, 3))
    vn = np.zeros((len(v), 3))
    dropped = np.zeros(F, dtype=bool)
    for i in range(F):
        A, B, C = v[f[i, 0]], v[f[i, 1]], v[f[i, 2]]
        ab, ac = B - A, C - A
        cr = np.array([ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]])
        if not (cr != 0).any():
            dropped[i] = True
            continue
        fn[i] = cr / np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])
    local = ((0, 1), (0, 2), (1, 2))
    sharers = {}
    for i in range(F):
        if dropped[i]:
            continue
        for a, b in local:
            key = (min(f[i, a], f[i, b]), max(f[i, a], f[i, b]))
            sharers.setdefault(key, []).append(i)
    sums = {}
    for key, lst in sharers.items():
        s = np.zeros(3)
        for i in lst:                                  # ascending face order (a face is listed once per local edge it has there)
            s = s + fn[i]
        sums[key] = s
    for i in range(F):
        if dropped[i]:
            continue
        for e, (a, b) in enumerate(local):
            en[i, e] = sums[(min(f[i, a], f[i, b]), max(f[i, a], f[i, b]))]
        P = [v[f[i, 0]], v[f[i, 1]], v[f[i, 2]]]
        for c in range(3):
            u, w = P[(c + 1) % 3] - P[c], P[(c + 2) % 3] - P[c]
            with np.errstate(all="ignore"):
                cosang = dot(u, w) / (np.sqrt(dot(u, u)) * np.sqrt(dot(w, w)))
                ang = np.arccos(np.minimum(np.maximum(cosang, -1.0), 1.0))
            vn[f[i, c]] = vn[f[i, c]] + ang * fn[i]
    return fn, en, vn, dropped


def closest_on_face(P, A, B, C):
    """P (N,3) against ONE face: (Q (N,3), feature (N,), D2 (N,)) by the header's region walk, first hit wins."""
    with np.errstate(all="ignore"):
        ab, ac = B - A, C - A
        ap, bp, cp = P - A, P - B, P - C
        d1, d2 = dot(ab, ap), dot(ac, ap)
        d3, d4 = dot(ab, bp), dot(ac, bp)
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        conds = [(0, (d1 <= 0) & (d2 <= 0)), (1, (d3 >= 0) & (d4 <= d3)), (3, (vc <= 0) & (d1 >= 0) & (d3 <= 0)),
                 (2, (d6 >= 0) & (d5 <= d6)), (4, (vb <= 0) & (d2 >= 0) & (d6 <= 0)),
                 (5, (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))]
        feat = np.full(len(P), 6)
        for fid, c in reversed(conds):
            feat = np.where(c, fid, feat)
        den = 1.0 / ((va + vb) + vc)
        cand = {0: np.broadcast_to(A, P.shape), 1: np.broadcast_to(B, P.shape), 2: np.broadcast_to(C, P.shape),
                3: A + (d1 / (d1 - d3))[:, None] * ab, 4: A + (d2 / (d2 - d6))[:, None] * ac,
                5: B + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[:, None] * (C - B),
                6: (A + (vb * den)[:, None] * ab) + (vc * den)[:, None] * ac}
        Q = np.zeros_like(P)
        for fid, q in cand.items():
            Q = np.where((feat == fid)[:, None], q, Q)
        d = P - Q
        return Q, feat, dot(d, d)


def query(points, verts, faces, tables=None, band=math.inf, orientation=1):
    """Brute force: (value float64 (N,), closest float32 (N,3), face int32 (N,), known bool (N,)); a far point: +band, NaN, -1."""
    v, f = widen(verts, faces)
    P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    fn, en, vn, dropped = tables if tables is not None else pseudonormals_loops(v, f)
    N = len(P)
    best = np.full(N, np.inf)
    bf = np.full(N, -1, dtype=np.int64)
    bfeat = np.zeros(N, dtype=np.int64)
    bq = np.zeros((N, 3))
    for i in range(len(f)):                              # ascending: a strict < keeps the lowest index on ties
        if dropped[i]:
            continue
        Q, feat, D2 = closest_on_face(P, v[f[i, 0]], v[f[i, 1]], v[f[i, 2]])
        better = D2 < best
        best = np.where(better, D2, best)
        bf = np.where(better, i, bf)
        bfeat = np.where(better, feat, bfeat)
        bq = np.where(better[:, None], Q, bq)
    known = (bf >= 0) & (best <= band * band)
    fi = np.maximum(bf, 0)
    nrm = np.where((bfeat == 6)[:, None], fn[fi],
                   np.where((bfeat >= 3)[:, None], en[fi, np.clip(bfeat - 3, 0, 2)], vn[f[fi, np.clip(bfeat, 0, 2)]]))
    with np.errstate(all="ignore"):
        neg = (dot(P - bq, nrm) * float(orientation) < 0) & (best != 0)
        val = np.where(best == 0, 0.0, np.where(neg, -np.sqrt(best), np.sqrt(best)))
    val = np.where(known, val, band)
    closest = np.where(known[:, None], bq, np.nan).astype(np.float32)
    return val, closest, np.where(known, bf, -1).astype(np.int32), known, neg & known


def grid_points(origin, spacing, shape):
    o = np.broadcast_to(np.asarray(origin, dtype=np.float64), (3,))
    s = np.broadcast_to(np.asarray(spacing, dtype=np.float64), (3,))
    ax = [o[a] + np.arange(shape[a], dtype=np.float64) * s[a] for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)


def far_fill(status):
    """status (X,Y,Z): 0 undecided, 1 decided +, 2 decided -.  Sweeps z, y, x; returns the negative mask of every vertex."""
    dec = status != 0
    neg = status == 2
    for axis in (2, 1, 0):
        d = np.moveaxis(dec, axis, -1)
        n = np.moveaxis(neg, axis, -1)
        L = d.shape[-1]
        for idx in np.ndindex(d.shape[:-1]):
            line_d, line_n = d[idx], n[idx]                # views
            first = -1
            for t in range(L):
                if line_d[t]:
                    first = t
                    break
            if first < 0:
                continue
            carry = bool(line_n[first])
            for t in range(L):
                if line_d[t]:
                    carry = bool(line_n[t])
                else:
                    line_d[t] = True
                    line_n[t] = carry
    return neg & dec                                      # whatever is still undecided is +


def grid(verts, faces, origin, spacing, shape, band, tables=None, orientation=1, dtype=np.float32):
    """(volume `dtype` (X,Y,Z), closest float32 (X,Y,Z,3), face int32 (X,Y,Z), known bool (X,Y,Z))."""
    shape = tuple(shape)
    if math.isfinite(band) and band < np.max(np.broadcast_to(np.asarray(spacing, dtype=np.float64), (3,))):
        raise ValueError("band < max(spacing)")
    val, closest, face, known, neg = query(grid_points(origin, spacing, shape), verts, faces, tables, band, orientation)
    val, known, neg = val.reshape(shape), known.reshape(shape), neg.reshape(shape)
    if math.isfinite(band):
        status = np.where(known, np.where(neg, 2, 1), 0)
        fneg = far_fill(status)
        val = np.where(known, val, np.where(fneg, -band, band))
    return val.astype(dtype), closest.reshape(shape + (3,)), face.reshape(shape), known


def grid_banded(verts, faces, origin, spacing, shape, band, tables=None, orientation=1, dtype=np.float32):
    """grid() for a finite band on a big mesh: each face is evaluated only at the grid vertices inside its box grown by
    band + one spacing (every vertex outside is farther than band from the face, so the face cannot be the winner of a known
    vertex, and a far vertex needs no winner).  Same result as grid(), same return values."""
    shape = tuple(shape)
    v, f = widen(verts, faces)
    fn, en, vn, dropped = tables if tables is not None else pseudonormals_loops(v, f)
    o = np.broadcast_to(np.asarray(origin, dtype=np.float64), (3,))
    s = np.broadcast_to(np.asarray(spacing, dtype=np.float64), (3,))
    ax = [o[a] + np.arange(shape[a], dtype=np.float64) * s[a] for a in range(3)]
    best = np.full(shape, np.inf)
    bf = np.full(shape, -1, dtype=np.int64)
    bfeat = np.zeros(shape, dtype=np.int64)
    bq = np.zeros(shape + (3,))
    for i in range(len(f)):
        if dropped[i]:
            continue
        tri = v[f[i]]
        sl = []
        for a in range(3):
            lo = np.searchsorted(ax[a], tri[:, a].min() - band - s[a], side="left")
            hi = np.searchsorted(ax[a], tri[:, a].max() + band + s[a], side="right")
            sl.append(slice(int(lo), int(hi)))
        sl = tuple(sl)
        P = np.stack(np.meshgrid(ax[0][sl[0]], ax[1][sl[1]], ax[2][sl[2]], indexing="ij"), axis=-1)
        if P.size == 0:
            continue
        Q, feat, D2 = closest_on_face(P.reshape(-1, 3), tri[0], tri[1], tri[2])
        D2, feat, Q = D2.reshape(P.shape[:3]), feat.reshape(P.shape[:3]), Q.reshape(P.shape)
        better = D2 < best[sl]
        best[sl] = np.where(better, D2, best[sl])
        bf[sl] = np.where(better, i, bf[sl])
        bfeat[sl] = np.where(better, feat, bfeat[sl])
        bq[sl] = np.where(better[..., None], Q, bq[sl])
    known = (bf >= 0) & (best <= band * band)
    fi = np.maximum(bf, 0)
    nrm = np.where((bfeat == 6)[..., None], fn[fi],
                   np.where((bfeat >= 3)[..., None], en[fi, np.clip(bfeat - 3, 0, 2)], vn[f[fi, np.clip(bfeat, 0, 2)]]))
    P = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)
    with np.errstate(all="ignore"):
        neg = (dot(P - bq, nrm) * float(orientation) < 0) & (best != 0) & known
        val = np.where(best == 0, 0.0, np.where(neg, -np.sqrt(best), np.sqrt(best)))
    fneg = far_fill(np.where(known, np.where(neg, 2, 1), 0))
    val = np.where(known, val, np.where(fneg, -band, band))
    closest = np.where(known[..., None], bq, np.nan).astype(np.float32)
    return val.astype(dtype), closest, np.where(known, bf, -1).astype(np.int32), known
