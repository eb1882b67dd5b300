"""K20 restated in numpy: dfh_raycast's semantics (include/dfusion_hip.h), operation by operation in float64, vectorised over the
pixels of a view.  Every operation here is one IEEE operation on float64 arrays (no dot products, no sums over axes: numpy
may reorder or fuse those), in the header's order, so the device and this file agree bit for bit and there is no tie class to
exclude: `raycast` reports excluded = 0 by construction, and the GPU tests compare every pixel.

Only the plain march is restated.  The skipping march is defined as "the same bits as the plain march" and is tested against
it on the device.
"""
import numpy as np

QNAN = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]


def inverse_views(lws):
    """[R^-1 | -R^-1 t] per view: what kernels.raycast_inverse_views computes."""
    out = []
    for lw in lws:
        m = np.asarray(lw, dtype=np.float64).reshape(3, 4)
        ri = np.linalg.inv(m[:, :3])
        out.append(np.concatenate([ri, -(ri @ m[:, 3:])], axis=1))
    return out


class Grid:
    """The slab [x0, x1) of a res grid that T (and Wt, C) hold."""

    def __init__(self, T, Wt=None, res=None, x_range=None, colors=None):
        self.T = np.asarray(T)
        self.Wt = None if Wt is None else np.asarray(Wt)
        self.res = tuple(int(r) for r in (self.T.shape if res is None else res))
        self.x0, self.x1 = (0, self.res[0]) if x_range is None else (int(x_range[0]), int(x_range[1]))
        assert self.T.shape == (self.x1 - self.x0, self.res[1], self.res[2])
        self.C = None if colors is None else np.asarray(colors, dtype=np.float32)
        self.has_cell = self.x1 - self.x0 >= 2 and self.res[1] >= 2 and self.res[2] >= 2


def value(g, p0, p1, p2, min_weight):
    """S(p): (known, t) for arrays of points."""
    lo0, m0, m1, m2 = float(g.x0), float(g.x1 - 2), float(g.res[1] - 2), float(g.res[2] - 2)
    with np.errstate(all="ignore"):
        c0, c1, c2 = np.floor(p0), np.floor(p1), np.floor(p2)
        c0 = np.where(c0 >= lo0, c0, lo0); c0 = np.where(c0 <= m0, c0, m0)
        c1 = np.where(c1 >= 0.0, c1, 0.0); c1 = np.where(c1 <= m1, c1, m1)
        c2 = np.where(c2 >= 0.0, c2, 0.0); c2 = np.where(c2 <= m2, c2, m2)
        f0, f1, f2 = p0 - c0, p1 - c1, p2 - c2
        i0, i1, i2 = c0.astype(np.int64) - g.x0, c1.astype(np.int64), c2.astype(np.int64)

        def corner(A, a, b, c):
            return A[i0 + a, i1 + b, i2 + c].astype(np.float64)
        known = np.ones(p0.shape, dtype=bool)
        if min_weight > 0.0:
            for a in (0, 1):
                for b in (0, 1):
                    for c in (0, 1):
                        known &= corner(g.Wt, a, b, c) >= min_weight
        u000, u001, u010, u011 = corner(g.T, 0, 0, 0), corner(g.T, 0, 0, 1), corner(g.T, 0, 1, 0), corner(g.T, 0, 1, 1)
        u100, u101, u110, u111 = corner(g.T, 1, 0, 0), corner(g.T, 1, 0, 1), corner(g.T, 1, 1, 0), corner(g.T, 1, 1, 1)
        dz00, dz01, dz10, dz11 = u001 - u000, u011 - u010, u101 - u100, u111 - u110
        e00, e01, e10, e11 = u000 + f2 * dz00, u010 + f2 * dz01, u100 + f2 * dz10, u110 + f2 * dz11
        h0, h1 = e00 + f1 * (e01 - e00), e10 + f1 * (e11 - e10)
        t = h0 + f0 * (h1 - h0)
    return known, t


def _color(g, p0, p1, p2, crossed):
    """dfh_sample_colors' rule at p, rounded to bytes: (n, 4) uint8."""
    n = p0.shape[0]
    out = np.zeros((n, 4), dtype=np.uint8)
    X, Y, Z = g.res
    with np.errstate(all="ignore"):
        inn = crossed & (p0 >= 0.0) & (p0 <= float(X - 1)) & (p1 >= 0.0) & (p1 <= float(Y - 1)) & (p2 >= 0.0) & (p2 <= float(Z - 1))
    idx = np.nonzero(inn)[0]
    if idx.size == 0:
        return out
    q0, q1, q2 = p0[idx], p1[idx], p2[idx]
    ix = np.maximum(np.minimum(np.floor(q0).astype(np.int64), X - 2), 0)
    iy = np.maximum(np.minimum(np.floor(q1).astype(np.int64), Y - 2), 0)
    iz = np.maximum(np.minimum(np.floor(q2).astype(np.int64), Z - 2), 0)
    fx, fy, fz = q0 - ix.astype(np.float64), q1 - iy.astype(np.float64), q2 - iz.astype(np.float64)
    S = np.zeros(idx.size); sr = np.zeros(idx.size); sg = np.zeros(idx.size); sb = np.zeros(idx.size)
    for corner in range(8):
        dx, dy, dz = corner >> 2, (corner >> 1) & 1, corner & 1
        cx, cy, cz = ix + dx, iy + dy, iz + dz
        ok = (cx >= g.x0) & (cx < g.x1) & (cy < Y) & (cz < Z)
        c = g.C[np.where(ok, cx - g.x0, 0), np.where(ok, cy, 0), np.where(ok, cz, 0)]
        ok &= c[:, 3] > np.float32(0.0)
        wx = fx if dx else 1.0 - fx
        wy = fy if dy else 1.0 - fy
        wz = fz if dz else 1.0 - fz
        tw = (wx * wy) * wz
        S = np.where(ok, S + tw, S)
        sr = np.where(ok, sr + tw * c[:, 0].astype(np.float64), sr)
        sg = np.where(ok, sg + tw * c[:, 1].astype(np.float64), sg)
        sb = np.where(ok, sb + tw * c[:, 2].astype(np.float64), sb)
    with np.errstate(all="ignore"):
        valid = S != 0.0
        for ch, s in enumerate((sr, sg, sb)):
            q = s / S
            b = np.where(q > 0.0, np.where(q >= 255.0, 255.0, np.rint(q)), 0.0)
            out[idx, ch] = np.where(valid, np.nan_to_num(b), 0.0).astype(np.uint8)
        out[idx, 3] = np.where(valid, 255, 0)
    return out


def raycast_view(g, Kinv, wl, H, W, scale, center, half, step=0.5, z_near=0.0, z_far=np.inf, min_weight=0.0, refine=1,
                 max_steps=1 << 20, want_color=False):
    """One view: dict(depth (H, W) f32, normals (H, W, 3) f32, hit (H, W, 3) f32, color (H, W, 4) u8 or None, samples (H, W) int:
    the samples the plain march evaluated, steps (H, W) int: kmax + 1)."""
    Kinv = np.asarray(Kinv, dtype=np.float64).reshape(3, 3)
    wl = np.asarray(wl, dtype=np.float64).reshape(3, 4)
    center = np.asarray(center, dtype=np.float64).reshape(3)
    scale, half = float(scale), float(half)
    n = H * W
    depth = np.zeros(n, dtype=np.float32)
    normals = np.zeros((n, 3), dtype=np.float32)
    hit = np.full((n, 3), QNAN, dtype=np.float32)
    color = np.zeros((n, 4), dtype=np.uint8) if want_color else None
    samples = np.zeros(n, dtype=np.int64)
    steps = np.zeros(n, dtype=np.int64)

    def done():
        return dict(depth=depth.reshape(H, W), normals=normals.reshape(H, W, 3), hit=hit.reshape(H, W, 3),
                    color=None if color is None else color.reshape(H, W, 4), samples=samples.reshape(H, W), steps=steps.reshape(H, W),
                    excluded=0)
    if not g.has_cell:
        return done()
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    X, Y = xx.reshape(-1).astype(np.float64), yy.reshape(-1).astype(np.float64)
    with np.errstate(all="ignore"):
        # 1. ray
        rho = [(Kinv[r, 0] * X + Kinv[r, 1] * Y) + Kinv[r, 2] for r in range(3)]
        d = [(wl[r, 0] * rho[0] + wl[r, 1] * rho[1]) + wl[r, 2] * rho[2] for r in range(3)]
        o = [np.full(n, (wl[a, 3] - center[a]) / scale + half) for a in range(3)]
        e = [d[a] / scale for a in range(3)]
        L = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        alive = (L > 0.0) & (L < np.inf)
        # 2. clip
        lo = [float(g.x0), 0.0, 0.0]
        hi = [float(g.x1 - 1), float(g.res[1] - 1), float(g.res[2] - 1)]
        zlo = np.full(n, float(z_near))
        zhi = np.full(n, float(z_far))
        for a in range(3):
            t1, t2 = (lo[a] - o[a]) / e[a], (hi[a] - o[a]) / e[a]
            tn, tf = np.where(t1 < t2, t1, t2), np.where(t1 < t2, t2, t1)
            zero = e[a] == 0.0
            alive &= ~zero | ((o[a] >= lo[a]) & (o[a] <= hi[a]))
            zlo = np.where(zero, zlo, np.where(tn > zlo, tn, zlo))
            zhi = np.where(zero, zhi, np.where(tf < zhi, tf, zhi))
        alive &= zlo <= zhi
        # 3. samples
        dz = step / L
        nd = np.floor((zhi - zlo) / dz)
        ms = min(int(max_steps), 1 << 30)
        kmax = np.where(alive, np.where(nd < float(ms), np.nan_to_num(nd, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64), ms), -1)
        steps[:] = kmax + 1
        # 4. walk
        za, ta, zb, tb = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        have = np.zeros(n, dtype=bool)
        crossed = np.zeros(n, dtype=bool)
        k = 0
        while True:
            idx = np.nonzero(~crossed & (k <= kmax))[0]
            if idx.size == 0:
                break
            z = zlo[idx] + float(k) * dz[idx]
            known, t = value(g, o[0][idx] + z * e[0][idx], o[1][idx] + z * e[1][idx], o[2][idx] + z * e[2][idx], min_weight)
            samples[idx] += 1
            cr = known & (t <= 0.0) & have[idx]
            ci, ni = idx[cr], idx[~cr]
            zb[ci], tb[ci] = z[cr], t[cr]
            crossed[ci] = True
            have[ni] = (known & (t > 0.0))[~cr]
            za[ni], ta[ni] = z[~cr], t[~cr]
            k += 1
        # 5. root
        idx = np.nonzero(crossed)[0]
        za, ta, zb, tb = za[idx], ta[idx], zb[idx], tb[idx]
        oo = [o[a][idx] for a in range(3)]
        ee = [e[a][idx] for a in range(3)]
        zs = za + (zb - za) * (ta / (ta - tb))
        going = np.ones(idx.size, dtype=bool)
        for _ in range(int(refine)):
            known, t = value(g, oo[0] + zs * ee[0], oo[1] + zs * ee[1], oo[2] + zs * ee[2], min_weight)
            going &= known
            pos = going & (t > 0.0)
            neg = going & ~(t > 0.0)
            za, ta = np.where(pos, zs, za), np.where(pos, t, ta)
            zb, tb = np.where(neg, zs, zb), np.where(neg, t, tb)
            zs = np.where(going, za + (zb - za) * (ta / (ta - tb)), zs)
        # 6. outputs
        p = [oo[a] + zs * ee[a] for a in range(3)]
        depth[idx] = (-zs).astype(np.float32)
        for a in range(3):
            hit[idx, a] = p[a].astype(np.float32)
        gvec = [np.zeros(idx.size) for _ in range(3)]
        ok = np.ones(idx.size, dtype=bool)
        for j in range(6):
            ax, sgn = j >> 1, (-1.0 if j & 1 else 1.0)
            q = [p[a] + sgn if a == ax else p[a] for a in range(3)]
            inside = np.ones(idx.size, dtype=bool)
            for a in range(3):
                inside &= (q[a] >= lo[a]) & (q[a] <= hi[a])
            known, t = value(g, q[0], q[1], q[2], min_weight)
            ok &= inside & known
            gvec[ax] = gvec[ax] + sgn * t
        sg = 1.0 if scale > 0.0 else -1.0
        m = [sg * ((wl[0, c] * gvec[0] + wl[1, c] * gvec[1]) + wl[2, c] * gvec[2]) for c in range(3)]
        l2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
        ok &= (l2 > 0.0) & (l2 < np.inf)
        ln = np.sqrt(l2)
        nh = [m[c] / ln for c in range(3)]
        r = [rho[c][idx] for c in range(3)]
        cdot = (nh[0] * (zs * r[0]) + nh[1] * (zs * r[1])) + nh[2] * (zs * r[2])
        flip = cdot > 0.0
        for c in range(3):
            v = np.where(flip, -nh[c], nh[c])
            normals[idx, c] = np.where(ok, v, 0.0).astype(np.float32)
        if want_color:
            color[idx] = _color(g, p[0], p[1], p[2], np.ones(idx.size, dtype=bool))
    return done()


def raycast(T, Wt, Kinv, wls, H, W, scale, center, half=None, res=None, x_range=None, colors=None, **kw):
    """All views: dict of stacked arrays (V, H, W, ...), plus excluded = 0."""
    g = Grid(T, Wt, res, x_range, colors)
    if half is None:
        half = g.res[0] / 2.0
    views = [raycast_view(g, Kinv, wl, H, W, scale, center, half, want_color=colors is not None, **kw) for wl in wls]
    out = {k: np.stack([v[k] for v in views]) for k in ("depth", "normals", "hit", "samples", "steps")}
    out["color"] = np.stack([v["color"] for v in views]) if colors is not None else None
    out["excluded"] = 0
    return out


def brick_table(T, x_range=None):
    """dfh_raycast_table restated: uint8 (nb0, nb1, nb2); T holds the slab's planes."""
    T = np.asarray(T).astype(np.float64)
    nx, Y, Z = T.shape
    nb = [(s + 7) // 8 for s in (nx, Y, Z)]
    out = np.zeros(nb, dtype=np.uint8)
    for b0 in range(nb[0]):
        for b1 in range(nb[1]):
            for b2 in range(nb[2]):
                blk = T[max(8 * b0 - 1, 0):8 * b0 + 10, max(8 * b1 - 1, 0):8 * b1 + 10, max(8 * b2 - 1, 0):8 * b2 + 10]
                mn, mx = blk.min(), blk.max()
                dead = bool(np.all(blk > 0.0)) and bool(mn > mx * 2.0 ** -30)
                out[b0, b1, b2] = 0 if dead else 1
    return out
