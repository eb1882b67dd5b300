"""Scenes for the K20 ray-cast tests (CPU and GPU): small volumes, cameras and settings, and the restatement's result for each,
computed once per process and shared."""
import functools
import math

import numpy as np

import raycast_np as RN

TD = 4.0                       # truncation, voxels


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """(lw, wl): a camera at `eye` looking at `target` along its +z axis; wl = [R^T | eye] is written down, not inverted."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = target - eye
    z = z / np.linalg.norm(z)
    x = np.cross(np.asarray(up, dtype=np.float64), z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    lw = np.concatenate([R, -(R @ eye)[:, None]], axis=1)
    wl = np.concatenate([R.T, eye[:, None]], axis=1)
    return lw, wl


def pinhole(f, cx, cy, skew=0.0, fy=None):
    K = np.array([[f, skew, cx], [0.0, f if fy is None else fy, cy], [0.0, 0.0, 1.0]])
    return K, np.linalg.inv(K)


def sphere(res, c, r, dtype=np.float32):
    i0, i1, i2 = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in res], indexing="ij")
    d = np.sqrt((i0 - c[0]) ** 2 + (i1 - c[1]) ** 2 + (i2 - c[2]) ** 2) - r
    return np.clip(d, -TD, TD).astype(dtype)


def plane(res, axis, level, sign=1.0, dtype=np.float32):
    """T = sign * (level - i_axis): sign = +1 is free space below `level`."""
    idx = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in res], indexing="ij")[axis]
    return np.clip(sign * (level - idx), -TD, TD).astype(dtype)


def cube(res, lo, hi, dtype=np.float32):
    """A solid cube [lo, hi]^3 in the Chebyshev metric: faces on the planes lo and hi."""
    idx = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in res], indexing="ij")
    mid, halfw = (lo + hi) / 2.0, (hi - lo) / 2.0
    d = np.maximum(np.maximum(np.abs(idx[0] - mid), np.abs(idx[1] - mid)), np.abs(idx[2] - mid)) - halfw
    return np.clip(d, -TD, TD).astype(dtype)


class Case:
    def __init__(self, name, T, K, Kinv, cams, H, W, scale, center, Wt=None, res=None, x_range=None, tsdf_res=None, colors=None, **kw):
        self.name = name
        self.T = np.ascontiguousarray(T)
        self.Wt = np.ones_like(self.T) if Wt is None else np.ascontiguousarray(Wt).astype(self.T.dtype)
        self.res = tuple(self.T.shape) if res is None else tuple(res)
        self.x_range = x_range
        self.tsdf_res = self.res[0] if tsdf_res is None else tsdf_res
        self.K, self.Kinv = K, Kinv
        self.lws = [c[0] for c in cams]
        self.wls = [c[1] for c in cams]
        self.H, self.W = H, W
        self.scale, self.center = scale, np.asarray(center, dtype=np.float64)
        self.colors = colors
        self.kw = kw

    def expected(self):
        return _expected(self.name)


SCALE, CENTER = 0.05, (0.1, -0.2, 2.0)


def world(i, res0, scale=SCALE, center=CENTER):
    return scale * (np.asarray(i, dtype=np.float64) - res0 / 2.0) + np.asarray(center)


def orbit(n, res, c, dist, elev=0.35):
    cams = []
    for j in range(n):
        a = 2.0 * math.pi * (j + 0.3) / n
        eye = np.asarray(c) + dist * np.array([math.cos(a) * math.cos(elev), math.sin(elev) * (1 if j % 2 else -1), math.sin(a) * math.cos(elev)])
        cams.append(look_at(world(eye, res[0]), world(c, res[0])))
    return cams


def dyadic_camera(eye_index, res0, scale, center):
    """Identity rotation, a camera at index point `eye_index` looking along +i_2: every entry a dyadic number."""
    eye = scale * (np.asarray(eye_index, dtype=np.float64) - res0 / 2.0) + np.asarray(center, dtype=np.float64)
    R = np.eye(3)
    return np.concatenate([R, -eye[:, None]], axis=1), np.concatenate([R, eye[:, None]], axis=1)


def _paint(res, x_range=None, hole=None):
    """A colour volume painted by position; wc = 0 inside `hole` ((lo, hi) per axis, index space)."""
    x0, x1 = (0, res[0]) if x_range is None else x_range
    i0, i1, i2 = np.meshgrid(np.arange(x0, x1, dtype=np.float32), np.arange(res[1], dtype=np.float32), np.arange(res[2], dtype=np.float32),
                             indexing="ij")
    C = np.stack([7.0 * i0 + 3.0, 250.0 - 6.0 * i1, 5.5 * i2 + 0.25 * i0, np.ones_like(i0)], axis=-1).astype(np.float32)
    if hole is not None:
        m = (i0 >= hole[0][0]) & (i0 <= hole[0][1]) & (i1 >= hole[1][0]) & (i1 <= hole[1][1]) & (i2 >= hole[2][0]) & (i2 <= hole[2][1])
        C[m, 3] = 0.0
    return np.ascontiguousarray(C)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    R32 = (32, 32, 32)
    c32 = (16.3, 15.6, 15.9)
    S32 = sphere(R32, c32, 10.0)
    K, Kinv = pinhole(40.0, 15.5, 11.5)
    out.append(Case("sphere_f32_3views", S32, K, Kinv, orbit(3, R32, c32, 34.0), 24, 32, SCALE, CENTER))
    Ks, Ksinv = pinhole(11.0, 4.2, 3.1, skew=0.7, fy=9.0)
    out.append(Case("sphere_f64_skewed_7x9", sphere(R32, c32, 10.0, np.float64), Ks, Ksinv, orbit(1, R32, c32, 30.0), 7, 9, SCALE, CENTER))
    K8, K8inv = pinhole(9.0, 3.6, 3.4)
    R24 = (24, 24, 24)
    out.append(Case("sphere_16views_8x8", sphere(R24, (12.2, 11.7, 12.1), 7.0), K8, K8inv, orbit(16, R24, (12.2, 11.7, 12.1), 26.0), 8, 8,
                    SCALE, CENTER))
    RG = (17, 20, 33)
    cg = (8.4, 9.7, 16.2)
    SG = sphere(RG, cg, 6.0)
    Kw, Kwinv = pinhole(30.0, 32.0, 4.0)
    out.append(Case("ragged_9x65", SG, Kw, Kwinv, orbit(3, RG, cg, 30.0), 9, 65, SCALE, CENTER))
    out.append(Case("slab_5_12", SG[5:12], Kw, Kwinv, orbit(3, RG, cg, 30.0), 9, 65, SCALE, CENTER, res=RG, x_range=(5, 12)))
    K1, K1inv = pinhole(10.0, 0.0, 0.0)
    out.append(Case("image_1x1", S32, K1, K1inv, [look_at(world((16.3, 15.6, -20.0), 32), world(c32, 32))], 1, 1, SCALE, CENTER))
    # dyadic: scale 2^-4, centre dyadic, f = 16, principal point (4, 4): pixel (4, 4) has rho = (0, 0, 1) exactly
    DS, DC = 0.0625, (0.5, -0.25, 2.0)
    Kd, Kdinv = pinhole(16.0, 4.0, 4.0)
    Kdinv = np.array([[0.0625, 0.0, -0.25], [0.0, 0.0625, -0.25], [0.0, 0.0, 1.0]])
    P24 = plane(R24, 2, 10.0)
    out.append(Case("dyadic_sphere", sphere(R24, (12.0, 12.0, 12.0), 7.0), Kd, Kdinv, [dyadic_camera((12.0, 12.0, -6.0), 24, DS, DC)], 8, 8,
                    DS, DC))
    out.append(Case("lattice_zeros_step1", P24, Kd, Kdinv, [dyadic_camera((12.0, 12.0, 2.0), 24, DS, DC)], 8, 8, DS, DC, step=1.0, refine=0))
    Wgap = np.ones(R24, dtype=np.float32)
    Wgap[:, :, 10] = 0.0
    out.append(Case("gap_min_weight_1", P24, Kd, Kdinv, [dyadic_camera((12.0, 12.0, 2.0), 24, DS, DC)], 8, 8, DS, DC, Wt=Wgap, step=1.0,
                    min_weight=1.0))
    out.append(Case("gap_min_weight_0", P24, Kd, Kdinv, [dyadic_camera((12.0, 12.0, 2.0), 24, DS, DC)], 8, 8, DS, DC, Wt=Wgap, step=1.0,
                    min_weight=0.0))
    out.append(Case("minus_to_plus", plane(R24, 2, 10.0, sign=-1.0), Kd, Kdinv,
                    [dyadic_camera((12.0, 12.0, 2.0), 24, DS, DC), look_at(world((3.0, 20.0, -9.0), 24, DS, DC), world((12.0, 12.0, 12.0), 24, DS, DC))],
                    8, 8, DS, DC))
    # a sphere in front of a wall: cameras inside the grid, inside the sphere, and with z_near beyond the sphere's front
    R40 = (40, 36, 40)
    cu = (20.0, 18.0, 16.0)
    U = np.minimum(sphere(R40, cu, 8.0), plane(R40, 2, 33.5))
    Ku, Kuinv = pinhole(14.0, 9.5, 7.5)
    tgt = world((20.0, 18.0, 33.0), 40)
    out.append(Case("camera_inside_grid", U, Ku, Kuinv, [look_at(world((20.5, 17.0, 3.0), 40), tgt)], 16, 20, SCALE, CENTER))
    out.append(Case("camera_inside_surface", U, Ku, Kuinv, [look_at(world((20.5, 17.0, 14.0), 40), tgt)], 16, 20, SCALE, CENTER))
    out.append(Case("z_near_beyond_surface", U, Ku, Kuinv, [look_at(world((20.5, 17.0, -20.0), 40), tgt)], 16, 20, SCALE, CENTER,
                    z_near=SCALE * 32.0))
    out.append(Case("max_steps_10", S32, K, Kinv, orbit(3, R32, c32, 34.0), 24, 32, SCALE, CENTER, max_steps=10))
    out.append(Case("refine_0", S32, K, Kinv, orbit(1, R32, c32, 34.0), 24, 32, SCALE, CENTER, refine=0))
    out.append(Case("refine_8", S32, K, Kinv, orbit(1, R32, c32, 34.0), 24, 32, SCALE, CENTER, refine=8))
    # surfaces exactly on brick faces and corners, and a volume without a live brick
    for lev in (7.0, 8.0, 9.0, 16.0):
        out.append(Case("plane_at_%d" % lev, plane(R24, 2, lev), Kd, Kdinv,
                        [dyadic_camera((12.0, 12.0, -8.0), 24, DS, DC), look_at(world((1.0, 5.0, -12.0), 24, DS, DC), world((12.0, 12.0, lev), 24, DS, DC))],
                        8, 8, DS, DC))
    out.append(Case("cube_8_16", cube(R24, 8.0, 16.0), K8, K8inv, orbit(3, R24, (12.0, 12.0, 12.0), 30.0), 8, 8, SCALE, CENTER))
    out.append(Case("all_free", np.full(R24, TD, dtype=np.float32), K8, K8inv, orbit(3, R24, (12.0, 12.0, 12.0), 30.0), 8, 8, SCALE, CENTER))
    # colour: painted by position, with an uncoloured region around part of the surface
    out.append(Case("colour", S32, K, Kinv, orbit(3, R32, c32, 34.0), 24, 32, SCALE, CENTER,
                    colors=_paint(R32, hole=((0, 31), (0, 14), (0, 31)))))
    out.append(Case("colour_slab", SG[5:12], Kw, Kwinv, orbit(3, RG, cg, 30.0), 9, 65, SCALE, CENTER, res=RG, x_range=(5, 12),
                    colors=_paint(RG, (5, 12))))
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = cases()[name]
    return RN.raycast(c.T, c.Wt, c.Kinv, c.wls, c.H, c.W, c.scale, c.center, half=c.tsdf_res / 2.0, res=c.res, x_range=c.x_range,
                      colors=c.colors, **c.kw)


def sphere_truth(c, centre, r):
    """Per view: (z_true (H, W), cos of the angle between ray and surface normal (H, W), |e| (H, W), analytic camera-space normal)."""
    out = []
    yy, xx = np.meshgrid(np.arange(c.H, dtype=np.float64), np.arange(c.W, dtype=np.float64), indexing="ij")
    for wl in c.wls:
        rho = np.stack([xx, yy, np.ones_like(xx)], axis=-1) @ c.Kinv.T
        e = (rho @ wl[:, :3].T) / c.scale
        o = (wl[:, 3] - c.center) / c.scale + c.tsdf_res / 2.0
        oc = o - np.asarray(centre)
        A = np.sum(e * e, axis=-1)
        B = e @ oc
        Cq = oc @ oc - r * r
        disc = B * B - A * Cq
        z = np.where(disc > 0, (-B - np.sqrt(np.maximum(disc, 0.0))) / A, np.nan)
        p = o + z[..., None] * e
        n_idx = (p - np.asarray(centre)) / r
        cosang = np.abs(np.sum(n_idx * e, axis=-1)) / np.sqrt(A)
        n_cam = np.sign(c.scale) * (n_idx @ wl[:, :3])          # R_wl^T n
        n_cam = n_cam / np.linalg.norm(n_cam, axis=-1, keepdims=True)
        out.append((z, cosang, np.sqrt(A), n_cam))
    return out


@functools.lru_cache(maxsize=None)
def roundtrip():
    """K1's oracle and back: the bench scene (sphere in front of a wall) seen by three quarter-size C1 cameras, fused into 32^3
    by oracle_np.fuse_depths, then cast from the same cameras with min_weight = 1.  Returns (case, depth maps (3, H, W) float64)."""
    from dynamicfusion_body_amd import scene
    from oracle import oracle_np as O
    H, W, f, cx, cy = 60, 80, 300.3113 / 4.0, 159.7033 / 4.0, 119.6003 / 4.0
    K = scene.intrinsics(f, cx, cy)
    Kinv = np.linalg.inv(K)
    res = 32
    scale, center, tdist = scene.grid_params(res)
    lws = [scene.view_extrinsic(a) for a in (-20.0, 0.0, 20.0)]
    depths = [scene.render_depth(K, lw, H, W, invalid_frac=0) for lw in lws]
    T = np.full((res, res, res), tdist / scale, dtype=np.float32)
    Wt = np.zeros_like(T)
    for d, lw in zip(depths, lws):
        O.fuse_depths(d, lw, K, Kinv, T, Wt, tdist, tsdf_res=res, scale=scale, center=center)
    cams = list(zip(lws, RN.inverse_views(lws)))
    c = Case("roundtrip_k1", T, K, Kinv, cams, H, W, scale, center, Wt=Wt, min_weight=1.0)
    return c, np.stack(depths)


def roundtrip_figures(cast_depth, depths):
    """(median, 95th percentile, count) of |cast - input| over the pixels valid in both, in the depth maps' units."""
    m = (cast_depth != 0) & (depths != 0)
    d = np.abs(cast_depth.astype(np.float64)[m] - depths[m])
    return float(np.median(d)), float(np.percentile(d, 95)), int(m.sum())
