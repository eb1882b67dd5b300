"""fp64 numpy restatement of the photometric term (include/dfusion_hip.h: dfh_gn_photometric) -- TEST INFRASTRUCTURE ONLY.

A photo sample is a canonical point p with a reference intensity ref: it is warped as a landmark is (tests/landmark_np.py), projected
into every view of a frame with the association's chain, depth-gated by fabs(sd) <= band_sd, and the row I(u, v) - ref of the view
with the smallest fabs(sd) is differentiated through the bilinear cell it falls into.  The Jacobian is the landmark term's axis row
with the axis e_a replaced by g = dI/dx' (held constant: the Gauss-Newton linearisation).  Pinned against central differences of the
rounding-free chain in tests/test_photometric_np.py; everything the device computes is compared with this file in
tests/test_gpu_photometric.py.

A frame is a dict: depth (list of H x W arrays, the maps as stored: z = -depth), color (list of H x W x 4 uint8 RGBX images), lw_cam
(list of 3 x 4), K, Kinv (3 x 3), scale, center (3,), half.
"""
import numpy as np

from oracle import gn_np as G
import landmark_np as LN


def luma(img):
    """Y = (77 R + 150 G + 29 B) / 256 of an H x W x 4 uint8 image: exact in fp64."""
    c = np.asarray(img).astype(np.int64)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2]).astype(np.float64) / 256.0


def gray_image(Y):
    """An RGBX image whose luma is the integer image Y exactly (R = G = B = Y: 77 + 150 + 29 = 256)."""
    Y = np.asarray(Y).astype(np.uint8)
    return np.stack([Y, Y, Y, np.full_like(Y, 255)], axis=-1)


def make_frame(depth, color, lw_cam, K, scale=1.0, center=(0.0, 0.0, 0.0), half=0.0, Kinv=None):
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    return {"depth": [np.asarray(d) for d in depth], "color": [np.asarray(c, dtype=np.uint8) for c in color],
            "lw_cam": [np.asarray(m, dtype=np.float64).reshape(3, 4) for m in lw_cam], "K": K,
            "Kinv": np.linalg.inv(K) if Kinv is None else np.asarray(Kinv, dtype=np.float64).reshape(3, 3),
            "scale": float(scale), "center": np.asarray(center, dtype=np.float64), "half": float(half)}


def project(xp, fr, view):
    """Step 2 up to the pixel: (lpos (L, 3), (a, b, c), u, v, visible) of the warped points in one view."""
    lw, K = fr["lw_cam"][view], fr["K"]
    pos = fr["scale"] * (xp - fr["half"]) + fr["center"]
    l = np.stack([((lw[i, 0] * pos[:, 0] + lw[i, 1] * pos[:, 1]) + lw[i, 2] * pos[:, 2]) + lw[i, 3] for i in range(3)], axis=1)
    a, b, c = ((K[i, 0] * l[:, 0] + K[i, 1] * l[:, 1]) + K[i, 2] * l[:, 2] for i in range(3))
    H, W = fr["depth"][view].shape
    with np.errstate(all="ignore"):
        u, v = a / c, b / c
        vis = (c != 0.0) & (u >= 0.0) & (u < W - 1) & (v >= 0.0) & (v < H - 1)
    return l, c, u, v, vis


def view_sd(fr, view, l, u, v, vis):
    """Step 2 from the pixel on: (sd (L,), valid (L,)): valid = visible, z > 0 and z u, z v finite."""
    Ki = fr["Kinv"]
    ui = np.where(vis, np.rint(np.where(vis, u, 0.0)), 0).astype(np.int64)
    vi = np.where(vis, np.rint(np.where(vis, v, 0.0)), 0).astype(np.int64)
    with np.errstate(all="ignore"):
        z = -1.0 * fr["depth"][view][vi, ui].astype(np.float64)
        a0, a1 = z * u, z * v
        ok = vis & (z > 0.0) & (a0 < np.inf) & (a1 < np.inf)
        sd = ((Ki[2, 0] * a0 + Ki[2, 1] * a1) + Ki[2, 2] * (z * 1.0)) - l[:, 2]
    return sd, ok


def bilinear(Y, u, v):
    """Step 4: (I, Iu, Iv) of the luma image Y at (u, v), which must be visible (0 <= u < W - 1, 0 <= v < H - 1)."""
    i0, j0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fu, fv = u - i0, v - j0
    Y00, Y10, Y01, Y11 = Y[j0, i0], Y[j0, i0 + 1], Y[j0 + 1, i0], Y[j0 + 1, i0 + 1]
    I = (1.0 - fv) * ((1.0 - fu) * Y00 + fu * Y10) + fv * ((1.0 - fu) * Y01 + fu * Y11)
    Iu = (1.0 - fv) * (Y10 - Y00) + fv * (Y11 - Y01)
    Iv = (1.0 - fu) * (Y01 - Y00) + fu * (Y11 - Y10)
    return I, Iu, Iv


def pulled_back_gradient(fr, view, c, u, v, Iu, Iv):
    """Step 6: g (L, 3) = dI/dx' = scale (Iu du/dlpos + Iv dv/dlpos) R."""
    K, R = fr["K"], fr["lw_cam"][view][:, :3]
    h = [Iu * ((K[0, j] - u * K[2, j]) / c) + Iv * ((K[1, j] - v * K[2, j]) / c) for j in range(3)]
    return np.stack([fr["scale"] * ((h[0] * R[0, i] + h[1] * R[1, i]) + h[2] * R[2, i]) for i in range(3)], axis=1)


def vector_jacobians(dqs, nbr, w, lw, bh, nb, p, g):
    """J (L, k, 6): d (g . x') / d xi of the k nodes' left twists with g (L, 3) constant -- landmark_np.axis_jacobians with e_a -> g."""
    dqs, lw = np.asarray(dqs, dtype=np.float64), np.asarray(lw, dtype=np.float64)
    qk = dqs[nbr]
    rl = lw[:4]
    rr, dd = bh[:, :4], bh[:, 4:]
    ra, da = qk[..., :4], qk[..., 4:]
    U = G.pure(G.qmul(G.qmul(G.qconj(rl), G.pure(g)), rl)[..., 1:])
    g_r = -2.0 * (G.qmul(G.qmul(U, rr), G.pure(p)) + G.qmul(U, dd))
    g_d = 2.0 * G.qmul(U, rr)
    gg = np.concatenate([g_r, g_d], axis=-1)
    gg = (gg - np.sum(gg * bh, axis=-1, keepdims=True) * bh) / nb[:, None]
    gr, gd = gg[:, None, :4], gg[:, None, 4:]
    Jw = 0.5 * (G.qmul(gr, G.qconj(ra)) + G.qmul(gd, G.qconj(da)))[..., 1:]
    Jv = 0.5 * G.qmul(gd, G.qconj(ra))[..., 1:]
    return np.asarray(w)[..., None] * np.concatenate([Jw, Jv], axis=-1)


def sample_views(xp, fr, band_sd):
    """Steps 2-4 and 6 for warped points xp: dict with view (L,; -1: none passed), sd, u, v, I, g (L, 3) of the chosen view."""
    L = len(xp)
    view = np.full(L, -1, dtype=np.int64)
    best = np.full(L, np.inf)
    out = {k: np.zeros(L) for k in ("sd", "u", "v", "I", "Iu", "Iv")}
    g = np.zeros((L, 3))
    for vw in range(len(fr["depth"])):
        l, c, u, v, vis = project(xp, fr, vw)
        sd, ok = view_sd(fr, vw, l, u, v, vis)
        with np.errstate(invalid="ignore"):
            take = ok & (np.abs(sd) <= band_sd) & (np.abs(sd) < best)
        if not take.any():
            continue
        sel = np.flatnonzero(take)
        I, Iu, Iv = bilinear(luma(fr["color"][vw]), u[sel], v[sel])
        g[sel] = pulled_back_gradient(fr, vw, c[sel], u[sel], v[sel], Iu, Iv)
        for k, val in (("sd", sd[sel]), ("u", u[sel]), ("v", v[sel]), ("I", I), ("Iu", Iu), ("Iv", Iv)):
            out[k][sel] = val
        best[sel] = np.abs(sd[sel])
        view[sel] = vw
    out["view"], out["g"] = view, g
    return out


def photo_rows(dqs, pos, ref, nbr, w, lw, fr, weight=1.0, conf=None, valid=None, huber_delta=0.0, max_diff=0.0, band_sd=np.inf,
               round_f32=True):
    """The term's rows at the node DQs `dqs`: dict with active (L,), view (L,; -1 inactive), resid (L,; unscaled, 0 inactive),
    r (L,) and J (L, k, 6) (scaled by sc, zero where inactive), obj (L,), and the chosen view's u, v, sd, I, g."""
    xp, bh, nb, p = LN.warp_points(dqs, pos, nbr, w, lw, round_f32)
    sv = sample_views(xp, fr, band_sd)
    ref = np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        r = sv["I"] - ref
        s2 = weight * (np.ones(len(ref)) if conf is None else np.asarray(conf, dtype=np.float64))
        act = (s2 > 0.0) & (sv["view"] >= 0) & (np.abs(r) < np.inf)
        if valid is not None:
            act &= np.asarray(valid) != 0
        if max_diff > 0.0:
            act &= np.abs(r) <= max_diff
    ra, s2a = np.where(act, r, 0.0), np.where(act, s2, 0.0)
    obj, sc = LN.huber(ra * ra, s2a, huber_delta)
    J = vector_jacobians(dqs, nbr, w, lw, bh, nb, p, sv["g"])
    out = dict(sv)
    out.update({"active": act, "view": np.where(act, sv["view"], -1), "resid": ra, "r": np.where(act, sc * ra, 0.0),
                "J": np.where(act[:, None, None], sc[:, None, None] * J, 0.0), "obj": np.where(act, obj, 0.0), "xp": xp,
                "view_any": sv["view"]})
    return out


def flat_rows(rows, nbr):
    """The active rows as data rows: (r (La,), J (La, k, 6), nbr (La, k))."""
    sel = np.flatnonzero(rows["active"])
    return rows["r"][sel], rows["J"][sel], nbr[sel]


def dense_term(N, rows, nbr):
    """Dense normal equations of the term alone: (J^T J (6N, 6N), the same assembly of |J|, J^T r (6N,), sum of obj)."""
    r, J, nb = flat_rows(rows, nbr)
    zero = (np.zeros((N, 0, 3)), np.zeros((N, 0), dtype=np.int64), np.zeros((N, 0, 3, 6)), np.zeros((N, 0, 3, 6)))
    A, b, _ = G.assemble_dense(N, r, J, nb, *zero)
    A_abs, _, _ = G.assemble_dense(N, np.abs(r), np.abs(J), nb, *zero)
    return A, A_abs, b, float(rows["obj"].sum())


def intensity_smooth(dqs, pos, nbr, w, lw, fr, view):
    """I of every point in a FIXED view through the rounding-free chain warp -> projection -> bilinear intensity (what the Jacobian
    is the derivative of, inside one cell)."""
    xp, _, _, _ = LN.warp_points(dqs, pos, nbr, w, lw, round_f32=False)
    out = np.zeros(len(pos))
    Ys = [luma(c) for c in fr["color"]]
    for vw in np.unique(view):
        sel = np.flatnonzero(view == vw)
        _, _, u, v, _ = project(xp[sel], fr, int(vw))
        out[sel] = bilinear(Ys[int(vw)], u, v)[0]
    return out


# ---------------------------------------------------------------- the recovery scene
RADIUS, CAM_DIST, IMG, FOCAL, PRINCIPAL = 6.0, 40.0, 128, 160.0, 63.5


def texture(points):
    """The texture painted on the cylinder, at canonical points: 128 + 60 sin(2 pi z / 8) + 40 sin(3 theta)."""
    th = np.arctan2(points[..., 1], points[..., 0])
    return 128.0 + 60.0 * np.sin(2.0 * np.pi * points[..., 2] / 8.0) + 40.0 * np.sin(3.0 * th)


def unslide_z(z, kind, amount=0.2):
    """The canonical z of a live z under landmark_np.slide."""
    if kind == "uniform":
        return z - amount
    k = amount / 16.0                                   # live = z + amount (z + 8) / 16 between z = -8 and z = 8
    mid = (z - 8.0 * k) / (1.0 + k)
    return np.where(z <= -8.0, z, np.where(z >= 8.0 + amount, z - amount, mid))


def camera(phi):
    """lw_cam (3 x 4) of a camera CAM_DIST from the axis at angle phi, looking at it: x = (-s, c, 0), y = (0, 0, -1), z = (-c, -s, 0)."""
    c, s = np.cos(phi), np.sin(phi)
    R = np.array([[-s, c, 0.0], [0.0, 0.0, -1.0], [-c, -s, 0.0]])
    C = CAM_DIST * np.array([c, s, 0.0])
    return np.concatenate([R, (-R @ C)[:, None]], axis=1)


def raycast(lw_cam, K, kind):
    """Analytic 8-bit intensity image (RGBX) and depth map (float32, z = -depth; 0 = nothing) of the slid textured cylinder."""
    R, t = lw_cam[:, :3], lw_cam[:, 3]
    C = -R.T @ t
    jj, ii = np.meshgrid(np.arange(IMG), np.arange(IMG), indexing="ij")
    d_cam = np.stack([(ii - K[0, 2]) / K[0, 0], (jj - K[1, 2]) / K[1, 1], np.ones_like(ii, dtype=np.float64)], axis=-1)
    d = d_cam @ R                                        # world direction R^T d_cam; the ray's parameter is the camera depth
    qa = d[..., 0] ** 2 + d[..., 1] ** 2
    qb = 2.0 * (C[0] * d[..., 0] + C[1] * d[..., 1])
    qc = C[0] ** 2 + C[1] ** 2 - RADIUS ** 2
    disc = qb * qb - 4.0 * qa * qc
    hit = disc > 0.0
    tt = np.where(hit, (-qb - np.sqrt(np.where(hit, disc, 0.0))) / (2.0 * qa), 0.0)
    P = C + tt[..., None] * d
    zc = unslide_z(P[..., 2], kind)
    hit &= (tt > 0.0) & (zc >= -10.0) & (zc <= 10.0)
    canon = np.stack([P[..., 0], P[..., 1], zc], axis=-1)
    Y = np.clip(np.rint(texture(canon)), 0, 255)
    depth = np.where(hit, -tt, 0.0).astype(np.float32)
    return gray_image(np.where(hit, Y, 0)), depth


def recovery_frame(kind):
    """Three pinhole views of 128^2, f = 160, c = 63.5, 40 voxels from the axis at 0, 120 and 240 degrees."""
    K = np.array([[FOCAL, 0.0, PRINCIPAL], [0.0, FOCAL, PRINCIPAL], [0.0, 0.0, 1.0]])
    cams = [camera(np.deg2rad(a)) for a in (0.0, 120.0, 240.0)]
    shots = [raycast(m, K, kind) for m in cams]
    return make_frame([s[1] for s in shots], [s[0] for s in shots], cams, K)


PHOTO_WEIGHT, BAND_SD = 1e-3, 0.5


def recovery_loop(s, fr, weight, pcg_iters=None, iters=None):
    """landmark_np.recovery_loop with the photometric rows of the solve's own samples in the landmark rows' place.  Returns (costs
    at every build, final dqs, active photo samples at the last build)."""
    N = s["N"]
    dqs = np.tile(s["lw"], (N, 1))
    wts = G.blend_weights(s["pos"], s["node_pos"][s["nbr"]], s["node_w"][s["nbr"]])
    ref = texture(s["pos"])
    costs, n_act = [], 0
    for _ in range(s["iters"] if iters is None else iters):
        r, J = G.data_residual_jacobian(dqs, s["pos"], s["nrm"], s["corr"], s["nbr"], s["node_pos"], s["node_w"], s["lw"])
        nbr = s["nbr"]
        cost = 0.5 * float(r @ r)
        if weight > 0.0:
            rows = photo_rows(dqs, s["pos"], ref, s["nbr"], wts, s["lw"], fr, weight=weight, band_sd=BAND_SD)
            rp, Jp, npn = flat_rows(rows, s["nbr"])
            r, J, nbr = np.concatenate([r, rp]), np.concatenate([J, Jp]), np.concatenate([nbr, npn])
            cost += float(rows["obj"].sum())
            n_act = int(rows["active"].sum())
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
    return costs, dqs, n_act


# ---------------------------------------------------------------- gates on representable boundaries
def boundary_scene():
    """Identity warp, scale 1, half = center 0, K = [[16, 0, cx], [0, 16, cy], [0, 0, 1]], camera = index space, points at z = 16:
    u = x + cx and v = y + cy exactly.  16 x 12 integer images Y[j][i] = 20 + 10 i + j, depth 16 everywhere (sd = 0)."""
    W, H, cx, cy = 16, 12, 7.5, 5.5
    node_pos = np.array([[0.0, 0, 16], [8, 0, 16], [0, 8, 16], [-8, -8, 16]])
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    Y = 20 + 10 * ii + jj
    return {"W": W, "H": H, "cx": cx, "cy": cy, "node_pos": node_pos, "node_w": np.full(4, 6.0), "knn": 2, "Y": Y,
            "dqs": np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0, 0]), (4, 1)), "lw": np.array([1.0, 0, 0, 0, 0, 0, 0, 0]),
            "lw_cam": np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)}


def boundary_frame(b, cx=None, depth=16.0, n_views=1, Ys=None):
    K = np.array([[16.0, 0, b["cx"] if cx is None else cx], [0, 16.0, b["cy"]], [0, 0, 1.0]])
    depth = list(depth) if isinstance(depth, (list, tuple)) else [depth] * n_views
    Ys = [b["Y"]] * n_views if Ys is None else Ys
    return make_frame([np.full((b["H"], b["W"]), -d, dtype=np.float32) for d in depth], [gray_image(y) for y in Ys],
                      [b["lw_cam"]] * n_views, K, Kinv=[[1.0 / 16, 0, -K[0, 2] / 16], [0, 1.0 / 16, -K[1, 2] / 16], [0, 0, 1.0]])


def boundary_cases():
    """(name, frame, pos (L, 3), ref (L,), valid, conf, settings, expected active (L,), expected view (L,)) of every gate on its
    boundary; positions are float32-exact, so the warp's roundings leave them where they are."""
    b = boundary_scene()
    below = lambda x: float(np.nextafter(x, -np.inf))
    at = lambda u, v: [u - b["cx"], v - b["cy"], 16.0]                    # the point that projects onto (u, v) with cx, cy
    Y = b["Y"]
    cases = []
    one = np.array([at(5.0, 4.0)])                                         # integer pixel: I = Y[4][5] = 74 exactly
    ref1 = np.array([float(Y[4, 5])])
    # u = W - 1 is out; the largest double below it (through cx: 7.5 + (7.5 - 2^-49)) is in; v = H - 1 is out
    edge = np.array([at(15.0, 4.0)])
    cases.append(("u = W-1", boundary_frame(b), edge, ref1, None, None, {}, [False], [-1]))
    cx_lo = below(15.0) - 7.5
    cases.append(("u just below W-1", boundary_frame(b, cx=cx_lo), edge, ref1, None, None, {}, [True], [0]))
    cases.append(("v = H-1", boundary_frame(b), np.array([at(5.0, 11.0)]), ref1, None, None, {}, [False], [-1]))
    cases.append(("u = 0", boundary_frame(b), np.array([at(0.0, 4.0)]), ref1, None, None, {}, [True], [0]))
    # fabs(sd) == band_sd is in (sd = 16.5 - 16)
    cases.append(("|sd| = band_sd", boundary_frame(b, depth=16.5), one, ref1, None, None, {"band_sd": 0.5}, [True], [0]))
    cases.append(("|sd| > band_sd", boundary_frame(b, depth=16.5), one, ref1, None, None, {"band_sd": below(0.5)}, [False], [-1]))
    cases.append(("sd = -band_sd", boundary_frame(b, depth=15.5), one, ref1, None, None, {"band_sd": 0.5}, [True], [0]))
    cases.append(("no depth", boundary_frame(b, depth=0.0), one, ref1, None, None, {}, [False], [-1]))
    # fabs(r) == max_diff is in (integer image, integer ref: r = 7 exactly)
    cases.append(("|r| = max_diff", boundary_frame(b), one, ref1 - 7.0, None, None, {"max_diff": 7.0}, [True], [0]))
    cases.append(("|r| > max_diff", boundary_frame(b), one, ref1 - 7.0, None, None, {"max_diff": below(7.0)}, [False], [-1]))
    cases.append(("r = -max_diff", boundary_frame(b), one, ref1 + 7.0, None, None, {"max_diff": 7.0}, [True], [0]))
    cases.append(("max_diff 0: no gate", boundary_frame(b), one, ref1 - 200.0, None, None, {"max_diff": 0.0}, [True], [0]))
    # what the term lists: NaN ref, conf 0, negative conf, valid 0 -- and one that stays
    five = np.array([at(3.0, 2.0), at(4.0, 3.0), at(5.0, 4.0), at(6.0, 5.0), at(7.0, 6.0)])
    cases.append(("flags", boundary_frame(b), five, np.array([np.nan, 50.0, 50.0, 50.0, 50.0]), [1, 1, 1, 0, 1], [1.0, 0.0, -2.0, 1.0, 0.5],
                  {}, [False, False, False, False, True], [-1, -1, -1, -1, 0]))
    # two views with equal |sd| (+0.25 and -0.25): index 0 wins, either way round; a strictly smaller |sd| in view 1 wins
    Y2 = [Y, Y + 3]
    cases.append(("tie +-", boundary_frame(b, depth=[16.25, 15.75], n_views=2, Ys=Y2), one, ref1, None, None, {"band_sd": 0.5}, [True], [0]))
    cases.append(("tie -+", boundary_frame(b, depth=[15.75, 16.25], n_views=2, Ys=Y2), one, ref1, None, None, {"band_sd": 0.5}, [True], [0]))
    cases.append(("view 1 nearer", boundary_frame(b, depth=[16.25, 16.125], n_views=2, Ys=Y2), one, ref1, None, None, {"band_sd": 0.5},
                  [True], [1]))
    cases.append(("view 0 out of band", boundary_frame(b, depth=[17.0, 16.25], n_views=2, Ys=Y2), one, ref1, None, None, {"band_sd": 0.5},
                  [True], [1]))
    return b, cases


# ---------------------------------------------------------------- the random fixture of the Jacobian and device tests
IDENT = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
LW = 1.03 * G.twist_exp_dq(np.array([0.01, -0.02, 0.015, 0.3, -0.2, 0.1]))          # a global warp with |r_lw| = 1.03
FIX_H, FIX_W = 12, 16


def fixture_frame(rng, n_views):
    """n_views cameras 30 units from the middle of the 10^3 sample box, swung about the y axis, a general 3 x 3 K (skew and a
    non-trivial last row), random 16 x 12 RGB images and float32 depth maps scattered about the box's depth (some pixels empty)."""
    scale, center, half = 0.9, np.array([0.2, -0.1, 0.3]), 0.5
    mid = scale * (np.full(3, 5.0) - half) + center
    K = np.array([[40.0, 0.3, 7.5], [0.1, 33.0, 5.5], [0.001, 0.002, 1.0]])
    cams, depth, color = [], [], []
    for a in (0.0, 0.3, -0.3, 0.15)[:n_views]:
        c, s = np.cos(a), np.sin(a)
        R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
        C = mid + 30.0 * np.array([s, 0.0, -c])
        cams.append(np.concatenate([R, (-R @ C)[:, None]], axis=1))
        d = -(30.0 + rng.uniform(-6.0, 6.0, size=(FIX_H, FIX_W)))
        d[rng.random((FIX_H, FIX_W)) < 0.1] = 0.0
        depth.append(d.astype(np.float32))
        color.append(rng.integers(0, 256, size=(FIX_H, FIX_W, 4), dtype=np.uint8))
    return make_frame(depth, color, cams, K, scale, center, half)


def near_decision(rows, fr, xp, band_sd, max_diff, huber_delta, tol=1e-9):
    """True where a sample's u, v, sd or r lies within `tol` (relative) of a boundary at which the chain decides: the image's
    edges, the pixel (rint) and cell (floor) boundaries, the band, a tie between two views, max_diff and the Huber delta."""
    near = lambda x, t: np.abs(x - t) <= tol * np.maximum(1.0, np.abs(t))
    bad = np.zeros(len(xp), dtype=bool)
    sds = []
    for vw in range(len(fr["depth"])):
        H, W = fr["depth"][vw].shape
        l, c, u, v, vis = project(xp, fr, vw)
        sd, ok = view_sd(fr, vw, l, u, v, vis)
        with np.errstate(invalid="ignore"):
            bad |= near(c, 0.0) | near(u, 0.0) | near(u, W - 1.0) | near(v, 0.0) | near(v, H - 1.0)
            bad |= vis & (near(2.0 * u, np.rint(2.0 * u)) | near(2.0 * v, np.rint(2.0 * v)))     # integers and half-integers
            if np.isfinite(band_sd):
                bad |= ok & near(np.abs(sd), band_sd)
        sds.append(np.where(ok, np.abs(sd), np.inf))
    for i in range(len(sds)):
        for j in range(i + 1, len(sds)):
            both = np.isfinite(sds[i]) & np.isfinite(sds[j])
            bad |= both & near(np.where(both, sds[i], 0.0), np.where(both, sds[j], 1.0))
    r = np.abs(rows["I"] - rows["ref_in"])
    with np.errstate(invalid="ignore"):
        if max_diff > 0.0:
            bad |= near(r, max_diff)
        if huber_delta > 0.0:
            bad |= near(r, huber_delta)
    return bad


def fixture(seed, knn, n, n_views, identity=False, cell_margin=0.0, band_sd=3.0, max_diff=0.0, huber_delta=0.0, one_tuple=False,
            seen_only=False):
    """A random graph of 12 nodes with n photo samples against n_views 16 x 12 views: dict with the graph, dqs, lw, the frame, pos,
    nrm, nbr, w and ref (= the sample's own intensity plus noise, so residuals are tens of intensity units).  Candidates within 1e-9
    of a decision boundary are rejected here, on the CPU; cell_margin > 0 also keeps fu, fv inside [margin, 1 - margin] (in every
    view that sees the sample)."""
    from oracle import oracle_np as O
    rng = np.random.default_rng(seed)
    N = 12
    node_pos = rng.uniform(0, 10, size=(N, 3))
    node_w = rng.uniform(3, 6, size=N)
    tw = rng.standard_normal((N, 6)) * np.array([0.02, 0.02, 0.02, 0.3, 0.3, 0.3])
    dqs = np.tile(IDENT, (N, 1)) if identity else G.apply_twists(np.tile(IDENT, (N, 1)), tw)
    lw = IDENT.copy() if identity else LW
    fr = fixture_frame(rng, n_views)
    centre = np.array([5.0, 6.0, 4.0])

    def tuples_of(pts):                                  # (one_tuple: the cluster's points all take the centre's nodes)
        if one_tuple:
            return np.tile(O.knn_bruteforce(centre[None], node_pos, knn), (len(pts), 1))
        return O.knn_bruteforce(pts, node_pos, knn)

    keep_pos, keep_ref = [], []
    have = 0
    while have < n:
        m = max(64, 2 * (n - have))
        pos = centre + 0.5 * rng.standard_normal((m, 3)) if one_tuple else rng.uniform(0.5, 9.5, size=(m, 3))
        pos = G.f32(pos)
        nbr = tuples_of(pos)
        w = G.blend_weights(pos, node_pos[nbr], node_w[nbr])
        rows = photo_rows(dqs, pos, np.zeros(m), nbr, w, lw, fr, band_sd=band_sd)
        ref = np.where(rows["view_any"] >= 0, rows["I"], 100.0) + 20.0 * rng.standard_normal(m)
        rows["ref_in"] = ref
        bad = near_decision(rows, fr, rows["xp"], band_sd, max_diff, huber_delta)
        if cell_margin > 0.0:
            for vw in range(n_views):
                _, _, u, v, vis = project(rows["xp"], fr, vw)
                fu, fv = u - np.floor(u), v - np.floor(v)
                with np.errstate(invalid="ignore"):
                    bad |= ~vis | (fu < cell_margin) | (fu > 1 - cell_margin) | (fv < cell_margin) | (fv > 1 - cell_margin)
        if seen_only:                                    # (only samples some view passes: a single sample must have a row)
            bad |= rows["view_any"] < 0
        keep_pos.append(pos[~bad])
        keep_ref.append(ref[~bad])
        have += int((~bad).sum())
    pos, ref = np.concatenate(keep_pos)[:n], np.concatenate(keep_ref)[:n]
    nbr = tuples_of(pos)
    nrm = rng.standard_normal((n, 3))
    return {"N": N, "knn": knn, "node_pos": node_pos, "node_w": node_w, "node_nbr": O.knn_bruteforce(node_pos, node_pos, knn), "dqs": dqs,
            "lw": lw, "frame": fr, "pos": pos, "nrm": nrm / np.linalg.norm(nrm, axis=1, keepdims=True), "nbr": nbr,
            "w": G.blend_weights(pos, node_pos[nbr], node_w[nbr]), "ref": ref, "band_sd": band_sd}
