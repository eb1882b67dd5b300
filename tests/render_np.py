"""numpy restatement of the rasterizer of csrc/dfh_render.hip (semantics: include/dfusion_hip.h, dfh_render_*).

Every fp64 expression is written in the kernel's operation order (numpy evaluates `a * b + c * d + e` left to right, without
fused multiply-adds, like the library built with -ffp-contract=off), so depth and face maps agree bit for bit.
The per-pixel work is vectorised over one triangle's box; triangles are visited one by one.
"""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def project(P, K, lw, scale, center, half):
    """(u, v, z) of points P (n,3) in voxel-index space."""
    P = np.asarray(P, dtype=np.float64)
    c = np.broadcast_to(np.asarray(center, dtype=np.float64), (3,))
    w0 = scale * (P[:, 0] - half) + c[0]
    w1 = scale * (P[:, 1] - half) + c[1]
    w2 = scale * (P[:, 2] - half) + c[2]
    r = np.asarray(lw, dtype=np.float64).reshape(-1)
    c0 = r[0] * w0 + r[1] * w1 + r[2] * w2 + r[3]
    c1 = r[4] * w0 + r[5] * w1 + r[6] * w2 + r[7]
    c2 = r[8] * w0 + r[9] * w1 + r[10] * w2 + r[11]
    K = np.asarray(K, dtype=np.float64)
    u = (K[0, 0] * c0 + K[0, 1] * c1 + K[0, 2] * c2) / c2
    v = (K[1, 1] * c1 + K[1, 2] * c2) / c2
    return u, v, c2


def edge(ua, va, ub, vb, x, y):
    """E_ab(x, y) evaluated from the lexicographically smaller end point (see the header)."""
    if ua < ub or (ua == ub and va < vb):
        return (x - ua) * (vb - va) - (y - va) * (ub - ua)
    return -((x - ub) * (va - vb) - (y - vb) * (ua - ub))


def setup(u, v, z, H, W, znear):
    """(A, x0, x1, y0, y1) or None if the triangle draws nothing."""
    with np.errstate(all="ignore"):
        if not all(z[i] > znear and np.isfinite(u[i]) and np.isfinite(v[i]) for i in range(3)):
            return None
        A = (u[2] - u[0]) * (v[1] - v[0]) - (v[2] - v[0]) * (u[1] - u[0])
        if not np.isfinite(A) or A == 0.0:
            return None
        xl = max(0.0, np.ceil(min(min(u[0], u[1]), u[2])))
        xh = min(float(W - 1), np.floor(max(max(u[0], u[1]), u[2])))
        yl = max(0.0, np.ceil(min(min(v[0], v[1]), v[2])))
        yh = min(float(H - 1), np.floor(max(max(v[0], v[1]), v[2])))
    if not (xl <= xh) or not (yl <= yh):
        return None
    return A, int(xl), int(xh), int(yl), int(yh)


def bary(u, v, A, xs, ys):
    """(covered mask, lambda0, lambda1, lambda2) at pixel centres (xs, ys)."""
    e0 = edge(u[1], v[1], u[2], v[2], xs, ys)
    e1 = edge(u[2], v[2], u[0], v[0], xs, ys)
    e2 = edge(u[0], v[0], u[1], v[1], xs, ys)
    if A > 0:
        inside = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
    else:
        inside = (e0 <= 0) & (e1 <= 0) & (e2 <= 0)
    return inside, e0 / A, e1 / A, e2 / A


def raster_triangle(u, v, z, H, W, znear):
    """One projected triangle: None if it draws nothing, else (x0, y0, covered mask over its box, fp64 z over its box,
    float32 z over its box)."""
    st = setup(u, v, z, H, W, znear)
    if st is None:
        return None
    A, x0, x1, y0, y1 = st
    ys, xs = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.float64), np.arange(x0, x1 + 1, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        inside, l0, l1, l2 = bary(u, v, A, xs, ys)
        s = l0 / z[0] + l1 / z[1] + l2 / z[2]
        z64 = 1.0 / s
        zf = z64.astype(np.float32)
    return x0, y0, inside & (s > 0) & np.isfinite(zf), z64, zf


def render(verts, faces, normals, K, lws, H, W, scale=1.0, center=0.0, half=0.0, znear=1e-3):
    """Same call shape and results as mesh.render, as numpy arrays: (depth (V,H,W) f32, normal (V,H,W,3) f32 or None,
    face (V,H,W) int32)."""
    verts = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    lws = np.asarray(lws, dtype=np.float64)
    if lws.ndim == 2:
        lws = lws[None]
    nv = len(lws)
    keys = np.full((nv, H, W), EMPTY, dtype=np.uint64)
    for vi in range(nv):
        with np.errstate(all="ignore"):
            U, Vv, Z = project(verts, K, lws[vi], scale, center, half)
        for f, (a, b, c) in enumerate(faces):
            if min(a, b, c) < 0 or max(a, b, c) >= len(verts):
                continue
            r = raster_triangle(U[[a, b, c]], Vv[[a, b, c]], Z[[a, b, c]], H, W, znear)
            if r is None:
                continue
            x0, y0, ok, _, zf = r
            key = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
            key = np.where(ok, key, EMPTY)
            blk = keys[vi, y0:y0 + ok.shape[0], x0:x0 + ok.shape[1]]
            np.minimum(blk, key, out=blk)
    hit = keys != EMPTY
    depth = np.where(hit, -(keys >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0)).astype(np.float32)
    face = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    normal = None
    if normals is not None:
        normals = np.asarray(normals, dtype=np.float64)
        normal = np.zeros((nv, H, W, 3), dtype=np.float32)
        for vi in range(nv):
            U, Vv, Z = project(verts, K, lws[vi], scale, center, half)
            r = lws[vi].reshape(-1)
            ys, xs = np.nonzero(hit[vi])
            for y, x in zip(ys, xs):
                f = int(face[vi, y, x])
                idx = faces[f]
                u, v, z = U[idx], Vv[idx], Z[idx]
                A = setup(u, v, z, H, W, znear)[0]
                _, l0, l1, l2 = bary(u, v, A, float(x), float(y))
                a0, a1, a2 = l0 / z[0], l1 / z[1], l2 / z[2]
                n0, n1, n2 = normals[idx[0]], normals[idx[1]], normals[idx[2]]
                m = [a0 * n0[j] + a1 * n1[j] + a2 * n2[j] for j in range(3)]
                n = [r[4 * j] * m[0] + r[4 * j + 1] * m[1] + r[4 * j + 2] * m[2] for j in range(3)]
                ln = np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
                if ln > 0:
                    normal[vi, y, x] = [n[0] / ln, n[1] / ln, n[2] / ln]
    return depth, normal, face
