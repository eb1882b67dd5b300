"""numpy restatement of the depth preprocessing kernel (csrc/dfh_depth_prep.hip; semantics: include/dfusion_hip.h, K12).

Element-wise float32 numpy: every `+ - * / sqrt` rounds once, like the kernel's scalar float32 operations (no fused
multiply-add, subnormals kept), and every expression is written in the header's operation order, so both outputs agree bit for
bit.  The tap loop is two Python loops over whole-image shifts, dy outer and dx inner: the accumulation order of the kernel."""
import numpy as np

F32 = np.float32


def valid(d):
    return np.isfinite(d) & (d < 0)


def bilateral(D, radius, spatial, range_lut, range_scale):
    """Stage A on one float32 map: F (H, W) float32."""
    D = np.asarray(D, dtype=F32)
    H, W = D.shape
    r = int(radius)
    v = valid(D)
    if r == 0:
        return np.where(v, D, F32(0))
    spatial = np.asarray(spatial, dtype=F32).reshape(2 * r + 1, 2 * r + 1)
    lut = np.asarray(range_lut, dtype=F32)
    s, nl = F32(range_scale), F32(len(lut))
    Dp = np.zeros((H + 2 * r, W + 2 * r), dtype=F32)
    vp = np.zeros((H + 2 * r, W + 2 * r), dtype=bool)
    Dp[r:r + H, r:r + W] = D
    vp[r:r + H, r:r + W] = v
    num = np.zeros((H, W), dtype=F32)
    den = np.zeros((H, W), dtype=F32)
    zero = F32(0)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                e = Dp[r + dy:r + dy + H, r + dx:r + dx + W]
                delta = e - D
                q = (delta * delta) * s
                ok = vp[r + dy:r + dy + H, r + dx:r + dx + W] & v & (q < nl)
                i = np.where(ok, q, zero).astype(np.int32)                # truncation
                w = spatial[dy + r, dx + r] * lut[i]
                num = num + np.where(ok, w * e, zero)
                den = den + np.where(ok, w, zero)
        pos = v & (den > 0)
        return np.where(pos, num / np.where(pos, den, F32(1)), zero).astype(F32)


def normals_of(F, Kinv, max_jump, min_cos):
    """Stage B on one filtered map: (normals (H, W, 3) float32 with zeros where there is none, classes), classes = dict of (H, W)
    bool maps: "has" (the pixel has a normal), "neighbour" (valid F, but a neighbour is outside, invalid or across a jump),
    "degenerate" (l2 == 0 or not finite), "grazing" (dropped by the cosine test)."""
    F = np.asarray(F, dtype=F32)
    H, W = F.shape
    Kf = np.asarray(Kinv, dtype=np.float64).reshape(3, 3).astype(F32)
    J = F32(max_jump)
    m2 = F32(min_cos) * F32(min_cos)
    x = np.arange(W, dtype=F32)[None, :]
    y = np.arange(H, dtype=F32)[:, None]
    vF = valid(F)
    nrm = np.zeros((H, W, 3), dtype=F32)
    cls = {k: np.zeros((H, W), dtype=bool) for k in ("has", "neighbour", "degenerate", "grazing")}
    with np.errstate(all="ignore"):
        z = -F
        P = [z * ((Kf[i, 0] * x + Kf[i, 1] * y) + Kf[i, 2]) for i in range(3)]
        c_ = (slice(1, H - 1), slice(1, W - 1))
        nbs = [(slice(1, H - 1), slice(0, W - 2)), (slice(1, H - 1), slice(2, W)), (slice(0, H - 2), slice(1, W - 1)),
               (slice(2, H), slice(1, W - 1))]                              # left, right, up, down
        ok = vF[c_].copy()
        for nb in nbs:
            ok &= vF[nb] & (np.abs(F[nb] - F[c_]) <= J)
        a = [P[i][nbs[1]] - P[i][nbs[0]] for i in range(3)]
        b = [P[i][nbs[3]] - P[i][nbs[2]] for i in range(3)]
        n0 = a[1] * b[2] - a[2] * b[1]
        n1 = a[2] * b[0] - a[0] * b[2]
        n2 = a[0] * b[1] - a[1] * b[0]
        l2 = (n0 * n0 + n1 * n1) + n2 * n2
        good = (l2 > 0) & np.isfinite(l2)
        ln = np.sqrt(l2)
        h = [n0 / ln, n1 / ln, n2 / ln]
        Pc = [P[i][c_] for i in range(3)]
        c = (h[0] * Pc[0] + h[1] * Pc[1]) + h[2] * Pc[2]
        flip = c > 0
        h = [np.where(flip, -hi, hi) for hi in h]
        c = np.where(flip, -c, c)
        pp = (Pc[0] * Pc[0] + Pc[1] * Pc[1]) + Pc[2] * Pc[2]
        keep = c * c >= m2 * pp
        has = ok & good & keep
    cls["has"][c_] = has
    cls["neighbour"] = vF.copy()
    cls["neighbour"][c_] &= ~ok
    cls["degenerate"][c_] = ok & ~good
    cls["grazing"][c_] = ok & good & ~keep
    for i in range(3):
        nrm[..., i][c_] = np.where(has, h[i], F32(0))
    return nrm, cls


def depth_prep(depths, Kinv, radius, spatial, range_lut, range_scale, max_jump, min_cos, mask=True, classes=None):
    """The whole call: depths = list of (H, W) float32 / float64 maps -> (clean (V, H, W), normals (V, H, W, 3)), float32.
    classes: optional list that receives one normals_of() class dict per view."""
    clean, normals = [], []
    for D in depths:
        D32 = np.asarray(D).astype(F32)                                     # float64: round to nearest even
        F = bilateral(D32, radius, spatial, range_lut, range_scale)
        nrm, cls = normals_of(F, Kinv, max_jump, min_cos)
        clean.append(np.where(cls["has"] | (not mask), F, F32(0)).astype(F32))
        normals.append(nrm)
        if classes is not None:
            classes.append(cls)
    return np.stack(clean), np.stack(normals)
