"""numpy restatement of dfh_integrate_color and dfh_sample_colors (K17) and the helpers their tests share.

integrate_color_np is warped_np.integrate_depth_dqb_np's chain for the warped position q, the pixel and the signed distance sd
-- the same oracle pieces (oracle_np.knn_bruteforce, oracle_np.warp), the same projection lines -- behind the canonical gate
(w > 0, |T| <= band_vox) and followed by the view gate |sd| <= band_sd and the colour running mean of include/dfusion_hip.h.
Beside the updated colour volume it returns the per-view masks and warped_np's margins (pixel, edge, sd, tie) plus one more,
  band  : | |sd| - band_sd | where the view has a measurement                (depth units)
so that a device comparison can leave out (and count) the voxels whose decision hangs on a last ulp.  The gate on T needs no
margin: both sides read the same stored numbers.
"""
import numpy as np

from oracle import oracle_np as O

import warped_np as WN


def integrate_color_np(C, T, Wt, depths, colors, lws, K, Kinv, scale, center, tdist, band_vox, band_sd, node_pos=None,
                       node_dq=None, node_w=None, knn=None, lw_dq=None, wmax=100.0, tsdf_res=None, x_range=None):
    """In place on C ((nx, Y, Z, 4) float32).  T, Wt: (nx, Y, Z) of any float dtype, read only.  colors: (H, W, >= 3) uint8.
    Returns (C, masks (V, nx, Y, Z) bool, margins dict of (nx, Y, Z) arrays; inf where a voxel is not live)."""
    assert C.dtype == np.float32 and C.shape == T.shape + (4,)
    K = np.asarray(K, dtype=np.float64)
    Kinv = np.asarray(Kinv, dtype=np.float64)
    center = np.asarray(center, dtype=np.float64)
    a, b = (0, T.shape[0]) if x_range is None else x_range
    assert b - a == T.shape[0]
    c = (T.shape[0] if tsdf_res is None else tsdf_res) / 2
    V = len(depths)
    masks = np.zeros((V,) + T.shape, dtype=bool)
    big = np.inf
    margins = {k: np.full(T.shape, big) for k in ("pixel", "edge", "sd", "tie", "band")}
    with np.errstate(invalid="ignore"):
        live = (Wt.astype(np.float64) > 0) & (np.abs(T.astype(np.float64)) <= band_vox)          # a NaN fails
    idx = np.nonzero(live)
    n = len(idx[0])
    if n == 0:
        return C, masks, margins
    pos = np.stack([idx[0] + a, idx[1], idx[2]], axis=-1).astype(np.float32).astype(np.float64)
    if node_pos is None:
        q = pos
    else:
        node_pos = np.asarray(node_pos, dtype=np.float64)
        node_dq = np.asarray(node_dq, dtype=np.float64)
        node_w = np.asarray(node_w, dtype=np.float64)
        q = np.empty_like(pos)
        tie = np.empty(n)
        for s in range(0, n, 4096):
            sl = slice(s, s + 4096)
            loc = O.knn_bruteforce(pos[sl], node_pos, knn)
            q[sl] = O.warp(pos[sl], node_dq[loc], node_pos[loc], node_w[loc], m_lw=lw_dq)
            x1 = O.dqb_warp(O.dq_blend(pos[sl], node_dq[loc], node_pos[loc], node_w[loc]), pos[sl])
            tie[sl] = np.min(WN.f32_tie_distance(x1), axis=-1)
        margins["tie"][idx] = tie
    mg = {k: np.full(n, big) for k in ("pixel", "edge", "sd", "band")}
    Cl = C[idx].copy()                                              # (n, 4) float32
    for v in range(V):
        dm, lw = np.asarray(depths[v]), np.asarray(lws[v], dtype=np.float64)
        img = np.asarray(colors[v])
        H, W = dm.shape
        assert img.dtype == np.uint8 and img.shape[:2] == (H, W)
        px = scale * (q[..., 0] - c) + center[0]
        py = scale * (q[..., 1] - c) + center[1]
        pz = scale * (q[..., 2] - c) + center[2]
        l0 = lw[0, 0] * px + lw[0, 1] * py + lw[0, 2] * pz + lw[0, 3]
        l1 = lw[1, 0] * px + lw[1, 1] * py + lw[1, 2] * pz + lw[1, 3]
        l2 = lw[2, 0] * px + lw[2, 1] * py + lw[2, 2] * pz + lw[2, 3]
        p0 = K[0, 0] * l0 + K[0, 1] * l1 + K[0, 2] * l2
        p1 = K[1, 0] * l0 + K[1, 1] * l1 + K[1, 2] * l2
        p2 = K[2, 0] * l0 + K[2, 1] * l1 + K[2, 2] * l2
        ok = p2 != 0
        p2s = np.where(ok, p2, 1.0)
        u = p0 / p2s
        vv = p1 / p2s
        vis = ok & (u >= 0) & (u < W - 1) & (vv >= 0) & (vv < H - 1)
        ui = np.where(vis, np.rint(u), 0).astype(np.int64)
        vi = np.where(vis, np.rint(vv), 0).astype(np.int64)
        z = -1 * dm[vi, ui].astype(np.float64)
        val = vis & (z > 0)
        with np.errstate(invalid="ignore", over="ignore"):
            cz = Kinv[2, 0] * (z * u) + Kinv[2, 1] * (z * vv) + Kinv[2, 2] * (z * 1.0)
            sd = cz - l2
            upd = val & (sd > -1 * tdist) & (np.abs(sd) <= band_sd)
        m = np.minimum(np.abs(u - np.floor(u) - 0.5), np.abs(vv - np.floor(vv) - 0.5))
        mg["pixel"] = np.minimum(mg["pixel"], np.where(vis, m, big))
        edge = np.minimum(np.minimum(np.abs(u), np.abs(u - (W - 1))), np.minimum(np.abs(vv), np.abs(vv - (H - 1))))
        mg["edge"] = np.minimum(mg["edge"], np.where(ok, edge, big))
        with np.errstate(invalid="ignore"):
            fin = val & np.isfinite(sd)
            mg["sd"] = np.minimum(mg["sd"], np.where(fin, np.abs(sd + tdist), big))
            mg["band"] = np.minimum(mg["band"], np.where(fin, np.abs(np.abs(sd) - band_sd), big))
        pix = img[vi, ui, :3].astype(np.float64)
        wc = Cl[:, 3].astype(np.float64)
        new = np.empty_like(Cl)
        for ch in range(3):
            new[:, ch] = ((Cl[:, ch].astype(np.float64) * wc + pix[:, ch]) / (wc + 1.0)).astype(np.float32)
        new[:, 3] = np.minimum(wc + 1.0, wmax).astype(np.float32)
        Cl = np.where(upd[:, None], new, Cl)
        masks[v][idx] = upd
    C[idx] = Cl
    for k in mg:
        margins[k][idx] = mg[k]
    return C, masks, margins


def excluded(margins):
    """The voxels left out of a device-against-numpy comparison: warped_np's rule, or a view whose |sd| sits on band_sd."""
    return WN.excluded(margins) | (margins["band"] < WN.SD_M)


def sample_colors_np(C, points, res=None, x_range=None):
    """dfh_sample_colors, statement for statement: (rgb (n, 3) float32, valid (n,) bool)."""
    points = np.asarray(points, dtype=np.float64)
    if res is None:
        res = C.shape[:3]
    x0, x1 = (0, res[0]) if x_range is None else x_range
    assert C.shape[0] == x1 - x0
    n = len(points)
    rgb = np.zeros((n, 3), dtype=np.float32)
    valid = np.zeros(n, dtype=bool)
    R = np.asarray(res, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        inside = np.all((points >= 0) & (points <= (R - 1)), axis=-1)
    p = np.where(inside[:, None], points, 0.0)
    i0 = np.maximum(np.minimum(np.floor(p).astype(np.int64), R - 2), 0)
    f = p - i0
    S = np.zeros(n)
    acc = np.zeros((n, 3))
    for corner in range(8):
        d = np.array([corner >> 2, (corner >> 1) & 1, corner & 1])
        ci = i0 + d
        counts = inside & (ci[:, 0] >= x0) & (ci[:, 0] < x1) & (ci[:, 1] < R[1]) & (ci[:, 2] < R[2])
        cs = np.where(counts[:, None], ci, [x0, 0, 0])
        pack = C[cs[:, 0] - x0, cs[:, 1], cs[:, 2]] if x1 > x0 else np.zeros((n, 4), dtype=np.float32)
        counts = counts & (pack[:, 3] > 0)
        w3 = np.where(d == 1, f, 1.0 - f)
        tw = (w3[:, 0] * w3[:, 1]) * w3[:, 2]
        S = np.where(counts, S + tw, S)
        with np.errstate(invalid="ignore", over="ignore"):
            for ch in range(3):
                acc[:, ch] = np.where(counts, acc[:, ch] + tw * pack[:, ch].astype(np.float64), acc[:, ch])
    valid = inside & (S != 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rgb = np.where(valid[:, None], acc / np.where(valid, S, 1.0)[:, None], 0.0).astype(np.float32)
    return rgb, valid


# ---------------------------------------------------------------------------------------------- the recovery scene
RECOVERY_RES, RECOVERY_ANGLES, RECOVERY_BAND = 32, (0.0, 40.0), 1.5


def analytic_color(world):
    """A smooth colour field over world positions ((..., 3) -> (..., 3) in [27.5, 227.5]): what the scene's surface is painted with."""
    x, y, z = world[..., 0], world[..., 1], world[..., 2]
    return np.stack([127.5 + 100.0 * np.sin(3.0 * x + 0.5), 127.5 + 100.0 * np.sin(3.0 * y - 1.0),
                     127.5 + 100.0 * np.sin(3.0 * z + 2.0)], axis=-1)


def recovery_scene():
    """The scene's sphere (no wall, every pixel measured) seen by camera C1 from 0 and 40 degrees, with colour images painted
    from analytic_color at each pixel's back-projected world position, and the grid FusionDM.compute_live_tsdf lays over it with
    UseAutoAlignment at 32^3 (its own arithmetic: centre = mean of the back-projected pixels, scale = 12 std / res); the
    truncation distance is 4 voxels of that grid."""
    from dynamicfusion_body_amd import FusionDM, scene
    H, W, fx, cx, cy = scene.CAMERAS["C1"]
    K = scene.intrinsics(fx, cx, cy)
    Kinv = np.linalg.inv(K)
    lws = [scene.view_extrinsic(a) for a in RECOVERY_ANGLES]
    depths = [scene.render_depth(K, lw, H, W, invalid_frac=0.0, dtype=np.float32, wall_z=None) for lw in lws]
    colors = []
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for d, lw in zip(depths, lws):
        z = -1.0 * d.astype(np.float64)
        cam = (z[..., None] * np.stack([u, v, np.ones_like(u)], axis=-1)) @ Kinv.T
        world = (cam - lw[:, 3]) @ lw[:, :3]                         # R^T (cam - t)
        img = np.zeros((H, W, 3), dtype=np.uint8)
        img[z > 0] = np.clip(np.rint(analytic_color(world[z > 0])), 0, 255).astype(np.uint8)
        colors.append(img)
    avg, std = FusionDM(1.0, K, tsdf_res=RECOVERY_RES)._auto_alignment(depths, lws)
    scale = 12 * std / RECOVERY_RES
    return dict(K=K, Kinv=Kinv, lws=lws, depths=depths, colors=colors, center=avg, scale=scale, tdist=4.0 * scale, res=RECOVERY_RES)


def recovery_metrics(s, verts, rgb, valid):
    """RMS error of the vertex colours against analytic_color at the vertices' world positions (valid vertices, all three
    channels) and the valid share."""
    world = s["scale"] * (np.asarray(verts, dtype=np.float64) - s["res"] / 2) + s["center"]
    err = np.asarray(rgb, dtype=np.float64)[valid] - analytic_color(world[valid])
    return {"rms": float(np.sqrt(np.mean(err * err))), "valid_share": float(np.mean(valid)), "n_vertices": int(len(verts))}


def recovery_colors(s, T, Wt, verts):
    """The restatement's colour volume from T, Wt (one call per view, no warp) and its samples at verts: (C, rgb, valid)."""
    C = np.zeros(T.shape + (4,), dtype=np.float32)
    for v in range(len(s["depths"])):
        integrate_color_np(C, T, Wt, s["depths"][v:v + 1], s["colors"][v:v + 1], s["lws"][v:v + 1], s["K"], s["Kinv"], s["scale"],
                           s["center"], s["tdist"], RECOVERY_BAND, RECOVERY_BAND * abs(s["scale"]), tsdf_res=s["res"])
    rgb, valid = sample_colors_np(C, verts)
    return C, rgb, valid


def recovery_record():
    """The whole chain in numpy: the oracle's fuse_depths on float64 volumes, its marching cubes at level 0, the colour
    restatement; what tests/golden/color_recovery.json records."""
    from oracle import mc_np
    s = recovery_scene()
    R = s["res"]
    T, Wt = np.zeros((R, R, R)) + s["tdist"], np.zeros((R, R, R))
    for d, lw in zip(s["depths"], s["lws"]):
        O.fuse_depths(d, lw, s["K"], s["Kinv"], T, Wt, s["tdist"], tsdf_res=R, scale=s["scale"], center=s["center"])
    verts = mc_np.marching_cubes(T, 0.0)[0]
    _, rgb, valid = recovery_colors(s, T, Wt, verts)
    return recovery_metrics(s, verts, rgb, valid)


# ---------------------------------------------------------------------------------------------- shared by the tests
def color_images(sc, seed=3):
    """Two different random RGBX images for the scene's two depth maps (every channel varies from pixel to pixel)."""
    rng = np.random.default_rng(seed)
    H, W = np.asarray(sc["depths"][0]).shape
    return [rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8) for _ in sc["depths"]]


def pattern(shape, seed=7):
    """A random non-zero colour volume: "untouched" is visible."""
    rng = np.random.default_rng(seed)
    C = rng.uniform(1.0, 250.0, size=tuple(shape) + (4,)).astype(np.float32)
    C[..., 3] = rng.integers(1, 5, size=tuple(shape)).astype(np.float32)
    return C


def restate(sc, knn, C, T, Wt, colors, band, warp=True, wmax=100.0, band_sd=None, depths=None, K=None, Kinv=None, x_range=None):
    """integrate_color_np on a warped_np scene; band in voxels, band_sd defaults to band * |scale|."""
    nodes = dict(node_pos=sc["node_pos"], node_dq=sc["node_dq"], node_w=sc["node_w"], knn=knn, lw_dq=sc["lw_dq"]) if warp else {}
    return integrate_color_np(C, T, Wt, sc["depths"] if depths is None else depths, colors, sc["lws"], sc["K"] if K is None else K,
                              sc["Kinv"] if Kinv is None else Kinv, sc["scale"], sc["center"], sc["tdist"], band,
                              band * abs(sc["scale"]) if band_sd is None else band_sd, wmax=wmax, tsdf_res=sc["tsdf_res"],
                              x_range=x_range, **nodes)
