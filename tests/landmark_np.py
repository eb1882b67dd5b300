"""fp64 numpy restatement of the landmark term (include/dfusion_hip.h: dfh_gn_landmarks) -- TEST INFRASTRUCTURE ONLY.

A landmark ties a canonical point p to a live 3-D target c with all three components of x' - c, where the data term has the one
row n'.(x' - c).  Built on oracle/gn_np.py: the warp is data_residual_jacobian's (the normalised static blend, warp_closed through
the blend and through lw, float32 roundings where Fusion.warp has them), and the Jacobian of axis a is that function's gradient with
the warped normal replaced by the constant axis e_a and its H (normal-rotation) term dropped.  The Jacobian is pinned against
central differences of the rounding-free warp in tests/test_landmark_np.py; everything the device computes is compared with this
file in tests/test_gpu_landmarks.py.

Rows of a landmark set are returned as (r (L, 3), J (L, 3, k, 6)); `flat_rows` turns them into 3 L one-component rows that the
assemblies of oracle/gn_np.py take beside the data rows.
"""
import numpy as np

from oracle import gn_np as G
from oracle import oracle_np as O


def warp_points(dqs, pos, nbr, w, lw, round_f32=True):
    """x' of every point (step 1), with the blend's pieces the Jacobian needs: (x', b^ (L, 8), |b|_8 (L,), p as it entered)."""
    dqs, lw = np.asarray(dqs, dtype=np.float64), np.asarray(lw, dtype=np.float64)
    b = np.sum(np.asarray(w, dtype=np.float64)[..., None] * dqs[nbr], axis=1)
    nb = np.sqrt(np.sum(b * b, axis=-1))
    bh = b / nb[:, None]
    rnd = G.f32 if round_f32 else (lambda a: np.asarray(a, dtype=np.float64))
    p = rnd(pos)
    x1 = G.warp_closed(bh, p)
    return G.warp_closed(lw, rnd(x1)), bh, nb, p


def axis_jacobians(dqs, nbr, w, lw, bh, nb, p):
    """J (L, 3, k, 6): d x'_a / d xi of the k nodes' left twists (step 5, unscaled)."""
    dqs, lw = np.asarray(dqs, dtype=np.float64), np.asarray(lw, dtype=np.float64)
    qk = dqs[nbr]
    rl = lw[:4]
    rr, dd = bh[:, :4], bh[:, 4:]
    ra, da = qk[..., :4], qk[..., 4:]
    out = []
    for a in range(3):
        U = G.pure(G.qmul(G.qmul(G.qconj(rl), G.pure(np.eye(3)[a])), rl)[1:])        # pure(vec(rl* e_a rl))
        g_r = -2.0 * (G.qmul(G.qmul(U, rr), G.pure(p)) + G.qmul(U, dd))
        g_d = 2.0 * G.qmul(U, rr)
        g = np.concatenate([g_r, g_d], axis=-1)
        g = (g - np.sum(g * bh, axis=-1, keepdims=True) * bh) / nb[:, None]
        gr, gd = g[:, None, :4], g[:, None, 4:]
        Jw = 0.5 * (G.qmul(gr, G.qconj(ra)) + G.qmul(gd, G.qconj(da)))[..., 1:]
        Jv = 0.5 * G.qmul(gd, G.qconj(ra))[..., 1:]
        out.append(np.asarray(w)[..., None] * np.concatenate([Jw, Jv], axis=-1))
    return np.stack(out, axis=1)


def gate(q, weight, conf=None, valid=None, max_dist=0.0):
    """(active (L,), s2 (L,)) of step 3 from the squared distances q."""
    q = np.asarray(q, dtype=np.float64)
    s2 = weight * (np.ones_like(q) if conf is None else np.asarray(conf, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        act = (s2 > 0.0) & (q < np.inf)
        if valid is not None:
            act &= np.asarray(valid) != 0
        if max_dist > 0.0:
            act &= q <= max_dist * max_dist
    return act, s2


def huber(q, s2, delta):
    """(objective, row scale sc) of step 4 for squared distances q and weights s2: vector Huber on |d|."""
    q, s2 = np.asarray(q, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    obj, sc = 0.5 * s2 * q, np.sqrt(s2)
    if delta > 0.0:
        out = q > delta * delta
        n = np.sqrt(np.where(out, q, 1.0))
        obj = np.where(out, s2 * delta * (n - 0.5 * delta), obj)
        sc = np.where(out, np.sqrt(s2) * np.sqrt(delta / n), sc)
    return obj, sc


def landmark_rows(dqs, pos, target, nbr, w, lw, weight=1.0, conf=None, valid=None, huber_delta=0.0, max_dist=0.0, round_f32=True):
    """The term's rows at the node DQs `dqs`: dict with active (L,), r (L, 3) and J (L, 3, k, 6) (scaled by sc, zero where
    inactive), obj (L,), d = x' - c and the warped points xp."""
    xp, bh, nb, p = warp_points(dqs, pos, nbr, w, lw, round_f32)
    d = xp - np.asarray(target, dtype=np.float64)
    q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    act, s2 = gate(q, weight, conf, valid, max_dist)
    qa, s2a = np.where(act, q, 0.0), np.where(act, s2, 0.0)
    obj, sc = huber(qa, s2a, huber_delta)
    J = axis_jacobians(dqs, nbr, w, lw, bh, nb, p)
    r = np.where(act[:, None], sc[:, None] * np.where(act[:, None], d, 0.0), 0.0)
    J = np.where(act[:, None, None, None], sc[:, None, None, None] * J, 0.0)
    return {"active": act, "r": r, "J": J, "obj": np.where(act, obj, 0.0), "d": d, "xp": xp}


def flat_rows(rows, nbr):
    """A landmark set's active rows as one-component data rows: (r (3 La,), J (3 La, k, 6), nbr (3 La, k))."""
    sel = np.flatnonzero(rows["active"])
    k = nbr.shape[1]
    return rows["r"][sel].reshape(-1), rows["J"][sel].reshape(-1, k, 6), np.repeat(nbr[sel], 3, axis=0)


def dense_term(N, rows, nbr):
    """Dense normal equations of the term alone: (J^T J (6N, 6N), the same assembly of |J|, J^T r (6N,), sum of obj)."""
    r, J, nb3 = flat_rows(rows, nbr)
    zero = (np.zeros((N, 0, 3)), np.zeros((N, 0), dtype=np.int64), np.zeros((N, 0, 3, 6)), np.zeros((N, 0, 3, 6)))
    A, b, _ = G.assemble_dense(N, r, J, nb3, *zero)
    A_abs, _, _ = G.assemble_dense(N, np.abs(r), np.abs(J), nb3, *zero)
    return A, A_abs, b, float(rows["obj"].sum())


def dense_data_and_reg(dqs, pos, nrm, corr, valid, nbr, node_nbr, node_pos, node_w, lw, rw, huber_delta=0.0):
    """Dense normal equations of the data rows and the regulariser (what a build leaves): (A, A_abs, b, objective)."""
    N = len(dqs)
    sel = np.flatnonzero(valid)
    r, J = G.data_residual_jacobian(dqs, pos[sel], nrm[sel], corr[sel], nbr[sel], node_pos, node_w, lw)
    obj = 0.5 * float(r @ r)
    if huber_delta > 0.0:
        sc, obj = G.huber_scale(r, huber_delta)
        r, J = r * sc, J * sc[:, None, None]
    rho, nb, Ji, Jj = G.reg_residual_jacobian(dqs, np.arange(N), node_nbr, node_pos, node_w, rw)
    A, b, _ = G.assemble_dense(N, r, J, nbr[sel], rho, nb, Ji, Jj)
    A_abs, _, _ = G.assemble_dense(N, np.abs(r), np.abs(J), nbr[sel], np.abs(rho), nb, np.abs(Ji), np.abs(Jj))
    return A, A_abs, b, obj + 0.5 * float(np.sum(rho * rho))


# ---------------------------------------------------------------- the recovery scene
def cylinder_points(n, rng, radius=6.0, z0=-10.0, z1=10.0):
    """n points uniform on the lateral surface of the cylinder about the z axis, with their radial normals."""
    th = rng.uniform(0.0, 2.0 * np.pi, n)
    z = rng.uniform(z0, z1, n)
    nrm = np.stack([np.cos(th), np.sin(th), np.zeros(n)], axis=1)
    return np.concatenate([radius * nrm[:, :2], z[:, None]], axis=1), nrm


def slide(points, kind, amount=0.2):
    """The motion the targets follow: along z by `amount`, everywhere ("uniform") or ramped as clip((z + 8) / 16, 0, 1)."""
    s = np.full(len(points), amount) if kind == "uniform" else amount * np.clip((points[:, 2] + 8.0) / 16.0, 0.0, 1.0)
    out = np.array(points, dtype=np.float64)
    out[:, 2] += s
    return out


def recovery_scene(kind, seed=16):
    """The cylinder sliding along its own axis: every plane row and every plane-row Jacobian entry of the axial translation is 0.
    Nodes on rings every 4 voxels, six per ring, node_w 8; 1 500 samples, 200 landmarks and 300 held-out points, knn 4.  All
    positions are float32-exact, so the roundings of the warp leave the canonical points where they are."""
    rng = np.random.default_rng(seed)
    ring = np.arange(6) * (np.pi / 3.0)
    node_pos = np.array([[6.0 * np.cos(t), 6.0 * np.sin(t), z] for z in np.arange(-10.0, 10.5, 4.0) for t in ring])
    node_pos = G.f32(node_pos)
    N, k = len(node_pos), 4
    node_w = np.full(N, 8.0)
    pos, nrm = cylinder_points(1500, rng)
    lpos, _ = cylinder_points(200, rng)
    hpos, hnrm = cylinder_points(300, rng)
    pos, nrm, lpos, hpos = G.f32(pos), G.f32(nrm), G.f32(lpos), G.f32(hpos)
    s = {"kind": kind, "N": N, "knn": k, "node_pos": node_pos, "node_w": node_w, "node_nbr": O.knn_bruteforce(node_pos, node_pos, k),
         "pos": pos, "nrm": nrm, "nbr": O.knn_bruteforce(pos, node_pos, k), "corr": slide(pos, kind),
         "lpos": lpos, "lnbr": O.knn_bruteforce(lpos, node_pos, k), "ltarget": slide(lpos, kind),
         "hpos": hpos, "hnrm": hnrm, "hnbr": O.knn_bruteforce(hpos, node_pos, k), "htruth": slide(hpos, kind),
         "lw": np.array([1.0, 0, 0, 0, 0, 0, 0, 0]), "rw": 0.2, "lm_abs": 1e-3, "lm_rel": 1e-2, "iters": 10}
    s["lwts"] = G.blend_weights(lpos, node_pos[s["lnbr"]], node_w[s["lnbr"]])
    s["hwts"] = G.blend_weights(hpos, node_pos[s["hnbr"]], node_w[s["hnbr"]])
    return s


def heldout_rms(s, dqs):
    """RMS over the held-out points of the tangential part of (warped point - true position): the error inside the surface."""
    xp, _, _, _ = warp_points(dqs, s["hpos"], s["hnbr"], s["hwts"], s["lw"])
    e = xp - s["htruth"]
    e = e - np.sum(e * s["hnrm"], axis=1, keepdims=True) * s["hnrm"]
    return float(np.sqrt(np.mean(np.sum(e * e, axis=1))))


def recovery_loop(s, weight, pcg_iters=None, iters=None, dqs=None):
    """The scene's Gauss-Newton loop: per iteration the plane rows of all samples (fixed corr), the regulariser, with weight > 0 the
    landmark rows, then the damped solve -- exact (pcg_iters None: sparse direct) or `pcg_iters` iterations of pcg_cg1 -- and the
    twist update.  Returns (costs at every build, final dqs)."""
    N = s["N"]
    dqs = np.tile(s["lw"], (N, 1)) if dqs is None else np.array(dqs, dtype=np.float64)
    costs = []
    for _ in range(s["iters"] if iters is None else iters):
        r, J = G.data_residual_jacobian(dqs, s["pos"], s["nrm"], s["corr"], s["nbr"], s["node_pos"], s["node_w"], s["lw"])
        nbr = s["nbr"]
        cost = 0.5 * float(r @ r)
        if weight > 0.0:
            rows = landmark_rows(dqs, s["lpos"], s["ltarget"], s["lnbr"], s["lwts"], s["lw"], weight=weight)
            rl, Jl, nl = flat_rows(rows, s["lnbr"])
            r, J, nbr = np.concatenate([r, rl]), np.concatenate([J, Jl]), np.concatenate([nbr, nl])
            cost += float(rows["obj"].sum())
        rho, nb, Ji, Jj = G.reg_residual_jacobian(dqs, np.arange(N), s["node_nbr"], s["node_pos"], s["node_w"], s["rw"])
        keys, blocks, Jtr, _ = G.assemble_blocks(N, r, J, nbr, rho, nb, Ji, Jj)
        costs.append(cost + 0.5 * float(np.sum(rho * rho)))
        if pcg_iters is None:
            import scipy.sparse.linalg as spla
            A = G.blocks_to_bsr(N, keys, G.damp_blocks(N, keys, blocks, s["lm_abs"], s["lm_rel"])).tocsc()
            dx = spla.spsolve(A, -Jtr.reshape(-1))
        else:
            dx = G.pcg_cg1(N, keys, blocks, Jtr, pcg_iters, s["lm_abs"], s["lm_rel"])
        dqs = G.apply_twists(dqs, dx.reshape(N, 6))
    return costs, dqs
