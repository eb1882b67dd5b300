"""numpy restatement of K21 (dfh_depth_halve, dfh_icp_track), in the operation order of include/dfusion_hip.h.

depth_halve is float32 element-wise, icp_rows float64 element-wise: both agree with the device bit for bit.  icp_sums adds the
rows with math.fsum (the exact sums the device's matrix-core sums are bounded against); icp_solve restates the damped Cholesky,
the guards and the SE(3) exponential on any 29 sums; icp_track chains whole iterations (numpy order of summation)."""
import math

import numpy as np

F32 = np.float32


def valid32(d):
    with np.errstate(invalid="ignore"):
        return (d < F32(0)) & (d > F32(-np.inf))


def depth_halve(D, max_jump):
    """(H, W) float32 / float64 -> (H//2, W//2) float32."""
    D = np.asarray(D)
    assert D.dtype in (np.float32, np.float64)
    D = D.astype(np.float32)
    H, W = D.shape
    Ho, Wo = H // 2, W // 2
    J = F32(max_jump)
    taps = [D[0:2 * Ho:2, 0:2 * Wo:2], D[0:2 * Ho:2, 1:2 * Wo:2], D[1:2 * Ho:2, 0:2 * Wo:2], D[1:2 * Ho:2, 1:2 * Wo:2]]
    a = taps[0]
    av = valid32(a)
    s = np.zeros((Ho, Wo), np.float32)
    n = np.zeros((Ho, Wo), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for e in taps:
            take = av & valid32(e) & (np.abs(e - a) <= J)
            s = np.where(take, s + e, s).astype(np.float32)
            n = np.where(take, n + F32(1), n).astype(np.float32)
        out = np.where(n > 0, s / np.where(n > 0, n, F32(1)), F32(0)).astype(np.float32)
    return out


def level_intrinsics(K):
    """The next coarser level's K (a pixel's coordinate is its integer index)."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    return np.array([[K[0, 0] / 2, K[0, 1] / 2, (K[0, 2] - 0.5) / 2], [0.0, K[1, 1] / 2, (K[1, 2] - 0.5) / 2], [0.0, 0.0, 1.0]])


def _rho(Kinv, X, Y):
    return [(Kinv[r, 0] * X + Kinv[r, 1] * Y) + Kinv[r, 2] for r in range(3)]


def icp_rows(Dl, Nl, Dm, Nm, K, Kinv, T, max_dist, min_cos, huber):
    """One view: (H, W, 8) float64 rows J0..5 | r | w, zeros where there is no row.  Nl may be None."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    Kinv = np.asarray(Kinv, np.float64).reshape(3, 3)
    T = np.asarray(T, np.float64).reshape(3, 4)
    Dl = np.asarray(Dl, np.float32)
    Dm = np.asarray(Dm, np.float32)
    Nm = np.asarray(Nm, np.float32).astype(np.float64)
    H, W = Dl.shape
    Y, X = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        ok = valid32(Dl)
        if Nl is not None:
            l = np.asarray(Nl, np.float32).astype(np.float64)
            l0, l1, l2 = l[..., 0], l[..., 1], l[..., 2]
            ll = (l0 * l0 + l1 * l1) + l2 * l2
            ok = ok & (ll > 0.0)
        d = Dl.astype(np.float64)
        rho = _rho(Kinv, X, Y)
        V = [(-d) * rho[r] for r in range(3)]
        P = [((T[r, 0] * V[0] + T[r, 1] * V[1]) + T[r, 2] * V[2]) + T[r, 3] for r in range(3)]
        q = [(K[r, 0] * P[0] + K[r, 1] * P[1]) + K[r, 2] * P[2] for r in range(3)]
        ok = ok & (q[2] > 0.0) & (q[2] < np.inf)
        ui = np.rint(q[0] / q[2])
        vi = np.rint(q[1] / q[2])
        ok = ok & (ui >= 0.0) & (ui <= float(W - 1)) & (vi >= 0.0) & (vi <= float(H - 1))
        uc = np.where(ok, ui, 0.0)
        vc = np.where(ok, vi, 0.0)
        iu = uc.astype(np.int64)
        iv = vc.astype(np.int64)
        mf = Dm[iv, iu]
        n = Nm[iv, iu]
        n0, n1, n2 = n[..., 0], n[..., 1], n[..., 2]
        nn = (n0 * n0 + n1 * n1) + n2 * n2
        ok = ok & valid32(mf) & (nn > 0.0)
        m = mf.astype(np.float64)
        s = _rho(Kinv, uc, vc)
        M = [(-m) * s[r] for r in range(3)]
        e = [P[r] - M[r] for r in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        if max_dist > 0.0:
            ok = ok & (d2 <= max_dist * max_dist)
        if Nl is not None:
            R = [(T[r, 0] * l0 + T[r, 1] * l1) + T[r, 2] * l2 for r in range(3)]
            c = (R[0] * n0 + R[1] * n1) + R[2] * n2
            mm = (R[0] * R[0] + R[1] * R[1]) + R[2] * R[2]
            ok = ok & (c > 0.0) & (c * c >= (min_cos * min_cos) * (mm * nn))
        r = (n0 * e[0] + n1 * e[1]) + n2 * e[2]
        J = [P[1] * n2 - P[2] * n1, P[2] * n0 - P[0] * n2, P[0] * n1 - P[1] * n0, n0, n1, n2]
        w = np.ones_like(r)
        if huber > 0.0:
            big = np.abs(r) > huber
            w = np.where(big, huber / np.where(big, np.abs(r), 1.0), 1.0)
        rows = np.stack(J + [r, w], axis=-1)
    return np.where(ok[..., None], rows, 0.0)


PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]


def icp_terms(rows):
    """(n_rows, 29) the per-row terms of the 29 sums (w J_i J_j | w J_i r | w r^2 | 1), of the pixels that have a row (w > 0)."""
    R = rows.reshape(-1, 8)
    R = R[R[:, 7] > 0.0]
    w = R[:, 7]
    cols = [w * R[:, i] * R[:, j] for i, j in PAIRS] + [w * R[:, i] * R[:, 6] for i in range(6)] + [w * R[:, 6] * R[:, 6], np.ones(len(R))]
    return np.stack(cols, axis=1) if len(R) else np.zeros((0, 29))


def icp_sums(rows, exact=True):
    """The 29 sums of one view's rows and, per entry, sum |term| (what the device's bound scales with)."""
    t = icp_terms(rows)
    if exact:
        s = np.array([math.fsum(t[:, k]) for k in range(29)])
    else:
        s = t.sum(axis=0)
    return s, np.array([math.fsum(np.abs(t[:, k])) for k in range(29)])


def se3_exp(xi):
    """(R, Vm, t) of the twist (omega, v), the header's expressions."""
    o = np.asarray(xi[:3], np.float64)
    v = np.asarray(xi[3:], np.float64)
    ww = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]
    if ww < 1e-8:
        a = 1.0 - ww / 6.0
        b = 0.5 - ww / 24.0
        c = 1.0 / 6.0 - ww / 120.0
    else:
        th = math.sqrt(ww)
        sn, cs = math.sin(th), math.cos(th)
        a = sn / th
        b = (1.0 - cs) / ww
        c = (th - sn) / (ww * th)
    Om = np.array([[0.0, -o[2], o[1]], [o[2], 0.0, -o[0]], [-o[1], o[0], 0.0]])
    R = np.zeros((3, 3))
    Vm = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            om2 = o[i] * o[j] - ww if i == j else o[i] * o[j]
            eye = 1.0 if i == j else 0.0
            R[i, j] = (eye + a * Om[i, j]) + b * om2
            Vm[i, j] = (eye + b * Om[i, j]) + c * om2
    t = np.array([(Vm[r, 0] * v[0] + Vm[r, 1] * v[1]) + Vm[r, 2] * v[2] for r in range(3)])
    return R, Vm, t


def apply_twist(xi, T):
    """exp(xi) T, a 3 x 4."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    R, _, t = se3_exp(xi)
    out = np.zeros((3, 4))
    for r in range(3):
        for c in range(4):
            m = (R[r, 0] * T[0, c] + R[r, 1] * T[1, c]) + R[r, 2] * T[2, c]
            out[r, c] = m + t[r] if c == 3 else m
    return out


def icp_solve(sums, T, lm_rel, min_count, max_rot, max_trans):
    """(status, xi, T') from 29 sums: the header's step 8 with Python floats (IEEE doubles, one rounding per operation)."""
    sums = [float(x) for x in sums]
    T = np.asarray(T, np.float64).reshape(3, 4)
    zero = np.zeros(6)
    if not sums[28] >= min_count:
        return 0, zero, T.copy()
    A = [[0.0] * 6 for _ in range(6)]
    for q, (i, j) in enumerate(PAIRS):
        A[i][j] = A[j][i] = sums[q]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = A[j][j] + lm_rel * A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not (s > 0.0 and s < math.inf):
            return 0, zero, T.copy()
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            t = A[i][j]
            for k in range(j):
                t = t - L[i][k] * L[j][k]
            L[i][j] = t / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        t = -sums[21 + i]
        for k in range(i):
            t = t - L[i][k] * y[k]
        y[i] = t / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        t = y[i]
        for k in range(i + 1, 6):
            t = t - L[k][i] * x[k]
        x[i] = t / L[i][i]
    ww = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]
    vv = (x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]
    if not (ww <= max_rot * max_rot and vv <= max_trans * max_trans):
        return 0, zero, T.copy()
    xi = np.array(x)
    return 1, xi, apply_twist(xi, T)


def icp_track(Dl, Nl, Dm, Nm, K, Kinv, T, max_dist, min_cos, huber, lm_rel, n_iters, min_count=6, max_rot=math.inf, max_trans=math.inf,
              exact=False):
    """n_iters iterations for one view: (T', stats (n_iters, 40)).  exact: the sums by math.fsum instead of numpy's order."""
    T = np.asarray(T, np.float64).reshape(3, 4).copy()
    stats = np.zeros((n_iters, 40))
    for it in range(n_iters):
        rows = icp_rows(Dl, Nl, Dm, Nm, K, Kinv, T, max_dist, min_cos, huber)
        sums, _ = icp_sums(rows, exact=exact)
        status, xi, T = icp_solve(sums, T, lm_rel, min_count, max_rot, max_trans)
        stats[it, :29] = sums
        stats[it, 29] = status
        stats[it, 30:36] = xi
    return T, stats


def invert_rigid(T):
    """[R^T | -R^T t] of a 3 x 4."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    return np.concatenate([T[:, :3].T, -(T[:, :3].T @ T[:, 3:])], axis=1)


def project_so3(R):
    """The nearest rotation (polar factor by SVD, det +1)."""
    u, _, vt = np.linalg.svd(np.asarray(R, np.float64))
    d = np.sign(np.linalg.det(u @ vt))
    return u @ np.diag([1.0, 1.0, d]) @ vt


def compose(A, B):
    """A B of two 3 x 4 rigid matrices."""
    A = np.asarray(A, np.float64).reshape(3, 4)
    B = np.asarray(B, np.float64).reshape(3, 4)
    return np.concatenate([A[:, :3] @ B[:, :3], A[:, :3] @ B[:, 3:] + A[:, 3:]], axis=1)
