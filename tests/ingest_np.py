"""The RGB-D ingest (K19, include/dfusion_hip.h: dfh_rgbd_ingest) restated in numpy from the header's text: the same operations
in the same order on float64 arrays, np.rint (half to even), float32 casts where the header has them, np.minimum.at for the
splat.  The GPU tests compare the device against this bit for bit on all outputs and on the z-buffer.

Also a small raw-frame generator: an analytic sphere-and-wall scene seen by a (distorted) depth camera and an offset colour
camera.  The generator inverts the distortion by fixed-point iteration when it draws distorted raw images; the stage itself
never needs the inverse."""
import numpy as np

EMPTY = np.uint32(0xffffffff)


def view(fd, kd=(0, 0, 0, 0, 0), fc=(1, 1, 0, 0), kc=(0, 0, 0, 0, 0), T=None):
    """One calibration record as the 5-tuple (fd[4], kd[5], fc[4], kc[5], T_dc[12]) of float64 arrays."""
    T = np.hstack([np.eye(3), np.zeros((3, 1))]) if T is None else T
    out = tuple(np.asarray(a, dtype=np.float64).reshape(-1) for a in (fd, kd, fc, kc, T))
    assert [a.size for a in out] == [4, 5, 4, 5, 12]
    return out


def distort(x, y, k):
    if not np.any(k != 0.0):
        return x, y
    k1, k2, p1, p2, k3 = (np.float64(c) for c in k)
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * rad + ((2.0 * p1) * (x * y) + p2 * (r2 + 2.0 * (x * x)))
    yd = y * rad + (p1 * (r2 + 2.0 * (y * y)) + (2.0 * p2) * (x * y))
    return xd, yd


def ideal(a, b, out_k):
    fx, fy, cx, cy = (np.float64(c) for c in out_k)
    return (a - cx) / fx, (b - cy) / fy


def decode(raw, fd, kd, out_k, depth_scale, z_min, z_max):
    """Stage A, steps 1-6 on the whole output grid: (valid (Hd, Wd) bool, z (Hd, Wd) float64)."""
    Hd, Wd = raw.shape
    j, i = np.meshgrid(np.arange(Hd, dtype=np.float64), np.arange(Wd, dtype=np.float64), indexing="ij")
    x, y = ideal(i, j, out_k)
    xd, yd = distort(x, y, fd_k(kd))
    us = fd[0] * xd + fd[2]
    vs = fd[1] * yd + fd[3]
    si, sj = np.rint(us), np.rint(vs)
    inside = (si >= 0.0) & (si <= Wd - 1.0) & (sj >= 0.0) & (sj <= Hd - 1.0)
    r = np.zeros((Hd, Wd), dtype=np.uint16)
    r[inside] = raw[sj[inside].astype(np.int64), si[inside].astype(np.int64)]
    z = r.astype(np.float64) * np.float64(depth_scale)
    valid = inside & (r != 0) & (z >= z_min) & ((z_max <= 0.0) | (z <= z_max))
    return valid, z


def fd_k(k):
    return np.asarray(k, dtype=np.float64)


def project(a, b, z, out_k, fc, kc, T):
    """Stage B, steps 1-6 for the points at pixel coordinates (a, b) and depth z: (in front, u, v, Pc_2)."""
    x, y = ideal(a, b, out_k)
    P0, P1 = x * z, y * z
    q = [((T[4 * r] * P0 + T[4 * r + 1] * P1) + T[4 * r + 2] * z) + T[4 * r + 3] for r in range(3)]
    front = q[2] > 0.0
    den = np.where(front, q[2], 1.0)
    xc, yc = q[0] / den, q[1] / den
    xd, yd = distort(xc, yc, fd_k(kc))
    u = fc[0] * xd + fc[2]
    v = fc[1] * yd + fc[3]
    return front, u, v, q[2]


def ingest(raw_depths, raw_colors, views, out_k, depth_scale=1e-3, z_min=0.0, z_max=0.0, occl_tol=0.0, max_splat=8, sample=1):
    """dfh_rgbd_ingest on numpy arrays: raw_depths (V, Hd, Wd) uint16, raw_colors None or (V, Hc, Wc, C) uint8, views a list of
    view() records -> (depth (V, Hd, Wd) float32, color (V, Hd, Wd, 4) uint8, color_depth (V, Hd, Wd) float32,
    zbuf (V, Hc, Wc) uint32); the last three None without colour."""
    raw_depths = np.asarray(raw_depths)
    V, Hd, Wd = raw_depths.shape
    assert raw_depths.dtype == np.uint16 and len(views) == V
    depth = np.zeros((V, Hd, Wd), dtype=np.float32)
    colour = raw_colors is not None
    if colour:
        raw_colors = np.asarray(raw_colors)
        assert raw_colors.dtype == np.uint8 and raw_colors.shape[0] == V and raw_colors.shape[3] in (3, 4)
        Hc, Wc = raw_colors.shape[1:3]
        color = np.zeros((V, Hd, Wd), dtype=np.uint32)
        cdepth = np.zeros((V, Hd, Wd), dtype=np.float32)
        zbuf = np.full((V, Hc, Wc), EMPTY, dtype=np.uint32)
    jj, ii = np.meshgrid(np.arange(Hd, dtype=np.float64), np.arange(Wd, dtype=np.float64), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for n, (fd, kd, fc, kc, T) in enumerate(views):
            valid, z = decode(raw_depths[n], fd, kd, out_k, depth_scale, z_min, z_max)
            depth[n] = np.where(valid, (-z).astype(np.float32), np.float32(0.0))
            if not colour:
                continue
            # ---- B: the splat ----
            f0, u0, v0, w0 = project(ii, jj, z, out_k, fc, kc, T)
            f1, u1, v1, _ = project(ii - 0.5, jj - 0.5, z, out_k, fc, kc, T)
            f2, u2, v2, _ = project(ii + 0.5, jj + 0.5, z, out_k, fc, kc, T)
            ok = valid & f0 & f1 & f2 & np.isfinite(u1) & np.isfinite(u2) & np.isfinite(v1) & np.isfinite(v2)
            a0 = np.maximum(np.rint(np.minimum(u1, u2)), 0.0)
            b0 = np.maximum(np.rint(np.minimum(v1, v2)), 0.0)
            a1 = np.minimum(np.minimum(np.rint(np.maximum(u1, u2)), Wc - 1.0), a0 + (max_splat - 1.0))
            b1 = np.minimum(np.minimum(np.rint(np.maximum(v1, v2)), Hc - 1.0), b0 + (max_splat - 1.0))
            ok &= (a0 <= a1) & (b0 <= b1)
            key = w0.astype(np.float32).view(np.uint32)
            zb = zbuf[n].reshape(-1)
            A0, A1, B0, B1, KEY = (t[ok] for t in (a0, a1, b0, b1, key))
            A0, A1, B0, B1 = (t.astype(np.int64) for t in (A0, A1, B0, B1))
            for dr in range(max_splat):
                for dc in range(max_splat):
                    m = (B0 + dr <= B1) & (A0 + dc <= A1)
                    if m.any():
                        np.minimum.at(zb, (B0[m] + dr) * Wc + (A0[m] + dc), KEY[m])
            # ---- C: the gather (the centre alone) ----
            inside = valid & f0 & (u0 >= 0.0) & (u0 < Wc - 1.0) & (v0 >= 0.0) & (v0 < Hc - 1.0)
            ru = np.where(inside, np.rint(u0), 0.0).astype(np.int64)
            rv = np.where(inside, np.rint(v0), 0.0).astype(np.int64)
            zf = zbuf[n][rv, ru].view(np.float32).astype(np.float64)
            occluded = zf + np.float64(occl_tol) < w0.astype(np.float32).astype(np.float64)
            has = inside & ~occluded
            img = raw_colors[n]
            if sample == 0:
                rgb = [img[rv, ru, c].astype(np.uint32) for c in range(3)]
            else:
                uu, vv = np.where(inside, u0, 0.0), np.where(inside, v0, 0.0)
                fi, fj = np.floor(uu), np.floor(vv)
                fu, fv = uu - fi, vv - fj
                i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
                rgb = []
                for c in range(3):
                    ch = img[:, :, c].astype(np.float64)
                    c00, c10, c01, c11 = ch[j0, i0], ch[j0, i0 + 1], ch[j0 + 1, i0], ch[j0 + 1, i0 + 1]
                    val = (1.0 - fv) * ((1.0 - fu) * c00 + fu * c10) + fv * ((1.0 - fu) * c01 + fu * c11)
                    rgb.append(np.rint(val).astype(np.int64).astype(np.uint32))
            packed = rgb[0] | rgb[1] << np.uint32(8) | rgb[2] << np.uint32(16) | np.uint32(255 << 24)
            color[n] = np.where(has, packed, np.uint32(0))
            cdepth[n] = np.where(has, depth[n], np.float32(0.0))
    if not colour:
        return depth, None, None, None
    return depth, color.view(np.uint8).reshape(V, Hd, Wd, 4), cdepth, zbuf


# ---- the raw-frame generator ---------------------------------------------------------------------------------------------------
SPHERE_RGB, WALL_RGB = (220, 40, 30), (20, 90, 230)
SPHERE, WALL = 1, 2


def undistort_points(xd, yd, k, iters=30):
    """The ideal (x, y) whose distort() is (xd, yd): fixed-point iteration x <- x - (distort(x) - xd) (converges for the mild
    coefficients the tests use)."""
    x, y = xd.copy(), yd.copy()
    k = fd_k(k)
    for _ in range(iters):
        ex, ey = distort(x, y, k)
        x, y = x - (ex - xd), y - (ey - yd)
    return x, y


def cast_rays(x, y, origin=(0.0, 0.0, 0.0), sphere=((0.0, 0.0, 2.0), 0.5), wall=3.0):
    """Rays origin + t*(x, y, 1) against the sphere (centre, radius) and the plane z = wall, all in the depth camera's frame:
    (z along the ray's own camera axis, label).  The colour camera is a pure translation of the depth camera."""
    o = np.asarray(origin, dtype=np.float64)
    c, rad = np.asarray(sphere[0], dtype=np.float64) - o, float(sphere[1])
    dd = x * x + y * y + 1.0
    dc = x * c[0] + y * c[1] + c[2]
    disc = dc * dc - dd * (c @ c - rad * rad)
    hit = disc >= 0.0
    t = np.where(hit, (dc - np.sqrt(np.where(hit, disc, 0.0))) / dd, np.inf)
    hit &= t > 0.0
    z = np.where(hit, t, wall - o[2])
    return z, np.where(hit, SPHERE, WALL).astype(np.uint8)


def pixel_rays(H, W, f4, k):
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    xd, yd = (i - f4[2]) / f4[0], (j - f4[3]) / f4[1]
    if np.any(fd_k(k) != 0.0):
        return undistort_points(xd, yd, k)
    return xd, yd


def raw_frame(depth_size, fd, kd, color_size, fc, kc, baseline, depth_scale=1e-3, **scene):
    """The scene through a depth camera at the origin and a colour camera `baseline` to its right (+x), both looking down +z:
    (raw depth (Hd, Wd) uint16, labels (Hd, Wd), z (Hd, Wd) float64 exact, raw colour (Hc, Wc, 3) uint8, T_dc (3, 4))."""
    x, y = pixel_rays(depth_size[0], depth_size[1], fd, kd)
    z, lab = cast_rays(x, y, **scene)
    raw = np.rint(z / depth_scale).astype(np.uint16)
    xc, yc = pixel_rays(color_size[0], color_size[1], fc, kc)
    _, clab = cast_rays(xc, yc, origin=(baseline, 0.0, 0.0), **scene)
    img = np.where((clab == SPHERE)[..., None], np.array(SPHERE_RGB, dtype=np.uint8), np.array(WALL_RGB, dtype=np.uint8))
    T = np.hstack([np.eye(3), np.array([[-baseline], [0.0], [0.0]])])
    return raw, lab, z, np.ascontiguousarray(img), T


def occlusion_scene():
    """The issue's scene: 160 x 120 depth at f 150, 320 x 240 colour at f 300, baseline 0.05, sphere of radius 0.5 at z 2, wall at 3,
    no distortion, output intrinsics = the raw depth camera's.  -> (raw, labels, img, view record, out_k)"""
    fd = (150.0, 150.0, 79.5, 59.5)
    fc = (300.0, 300.0, 159.5, 119.5)
    raw, lab, _, img, T = raw_frame((120, 160), fd, (0,) * 5, (240, 320), fc, (0,) * 5, 0.05)
    return raw, lab, img, view(fd, (0,) * 5, fc, (0,) * 5, T), fd


def occlusion_counts(occl_tol, sample=1, max_splat=8):
    """On occlusion_scene(): (wall pixels whose registered colour is the sphere's, pixels with a colour, correctly coloured
    pixels as a bool map).  "The sphere's": nearer the sphere's red than the wall's."""
    raw, lab, img, rec, out_k = occlusion_scene()
    _, color, _, _ = ingest(raw[None], img[None], [rec], out_k, occl_tol=occl_tol, sample=sample, max_splat=max_splat)
    color = color[0]
    has = color[..., 3] == 255
    is_sphere = color[..., 0].astype(np.int64) * 2 > SPHERE_RGB[0] + WALL_RGB[0]
    wrong_wall = has & (lab == WALL) & is_sphere
    correct = has & (((lab == WALL) & ~is_sphere) | ((lab == SPHERE) & is_sphere))
    return int(wrong_wall.sum()), int(has.sum()), correct
