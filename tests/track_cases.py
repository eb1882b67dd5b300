"""The tracking tests' scene, analytic and in numpy: two spheres of different radii in front of a tilted wall, seen through a
160 x 120 pinhole with f = 150.  The spheres' centres do not lie on one normal of the wall, so no rotation about an axis and no
translation along a direction leaves the depth maps unchanged (the sphere-and-wall scene of scene.py is symmetric about the camera
axis: a rotation about it cannot be recovered).  Units are metres; a depth map stores -z, 0 where a ray hits nothing."""
import math

import numpy as np

import depth_prep_np
import track_np

H, W, F = 120, 160, 150.0
K = np.array([[F, 0.0, (W - 1) / 2.0], [0.0, F, (H - 1) / 2.0], [0.0, 0.0, 1.0]])

SPHERES = [(np.array([-0.28, -0.10, 1.10]), 0.22), (np.array([0.33, 0.16, 1.35]), 0.14)]
WALL_N = np.array([0.25, -0.15, -1.0]) / np.linalg.norm([0.25, -0.15, -1.0])      # faces the camera at the origin
WALL_P = np.array([0.0, 0.0, 1.9])

IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)

# the schedule of the qualitative bar, finest level first
GATES = (0.1, 0.2, 0.4)
COSINES = (0.8, 0.65, 0.5)
ITERS = (4, 5, 10)
MAX_JUMP = 0.05
LM_REL = 1e-3


def pose(rot_deg, axis, trans):
    """world -> camera 3 x 4 of a camera rotated by rot_deg about `axis` and moved by `trans` from the identity."""
    T = track_np.apply_twist(np.concatenate([math.radians(rot_deg) * np.asarray(axis, float) / np.linalg.norm(axis), np.zeros(3)]), IDENT)
    T[:, 3] = np.asarray(trans, float)
    return T


def motion(size):
    """The applied motion of a given size (1 = 4.5 degrees and 111 mm): the camera that took the live frame."""
    return pose(4.5 * size, (0.3, 1.0, 0.2), 0.111 * size * np.array([0.6, -0.3, 0.74]) / np.linalg.norm([0.6, -0.3, 0.74]))


def render(lw, Kl=K, h=H, w=W):
    """(depth (h, w) float32, normals (h, w, 3) float32: camera space, facing the camera, zeros where nothing is hit) of the scene
    seen by the camera lw (world -> camera) through Kl."""
    lw = np.asarray(lw, float).reshape(3, 4)
    R, t = lw[:, :3], lw[:, 3]
    Kinv = np.linalg.inv(Kl)
    Y, X = np.meshgrid(np.arange(h, dtype=float), np.arange(w, dtype=float), indexing="ij")
    rho = np.stack([Kinv[r, 0] * X + Kinv[r, 1] * Y + Kinv[r, 2] for r in range(3)], axis=-1)        # camera point = z rho
    best = np.full((h, w), np.inf)
    nrm = np.zeros((h, w, 3))
    for c, rad in SPHERES:
        cc = R @ c + t                                                                              # centre in camera space
        a = (rho * rho).sum(-1)
        b = rho @ cc
        disc = b * b - a * (cc @ cc - rad * rad)
        with np.errstate(invalid="ignore"):
            z = (b - np.sqrt(disc)) / a
        hit = (disc > 0) & (z > 0) & (z < best)
        n = (z[..., None] * rho - cc) / rad
        best = np.where(hit, z, best)
        nrm = np.where(hit[..., None], n, nrm)
    wn, wp = R @ WALL_N, R @ WALL_P + t
    den = rho @ wn
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (wp @ wn) / den
    hit = (np.abs(den) > 1e-9) & (z > 0) & (z < best)
    best = np.where(hit, z, best)
    nrm = np.where(hit[..., None], wn, nrm)
    got = np.isfinite(best)
    flip = ((nrm * rho).sum(-1) > 0)[..., None]
    nrm = np.where(flip, -nrm, nrm)
    depth = np.where(got, -best, 0.0).astype(np.float32)
    return depth, np.where(got[..., None], nrm, 0.0).astype(np.float32)


def live_pyramid(depth, levels, Kl=K, max_jump=MAX_JUMP):
    """[(K_l, depth_l, normals_l)] finest first: CameraTracker.live_pyramid in numpy (depth_halve, then depth_prep's stage B with
    radius 0, min_cos 0, no mask at every level)."""
    out = []
    D = np.asarray(depth, np.float32)
    for l in range(levels):
        if l > 0:
            D = track_np.depth_halve(D, max_jump * 2.0 ** (l - 1))
            Kl = track_np.level_intrinsics(Kl)
        n, _ = depth_prep_np.normals_of(D, np.linalg.inv(Kl), max_jump * 2.0 ** l, 0.0)
        out.append((Kl, D, n))
    return out


def track_np_pyramid(live_depth, lw_prev, levels, gates, cosines, iters, huber=0.0, lm_rel=LM_REL, min_count=100, max_rot=0.5, max_trans=0.5,
                     model=render):
    """The restatement's coarse-to-fine track of one view: T (live camera -> model camera), the per-level stats (finest first)."""
    pyr = live_pyramid(live_depth, levels)
    T = IDENT.copy()
    stats = [None] * levels
    for l in range(levels - 1, -1, -1):
        Kl, D, n = pyr[l]
        md, mn = model(lw_prev, Kl, D.shape[0], D.shape[1])
        T, stats[l] = track_np.icp_track(D, n, md, mn, Kl, np.linalg.inv(Kl), T, gates[l], cosines[l], huber, lm_rel, iters[l],
                                         min_count=min_count, max_rot=max_rot, max_trans=max_trans)
    return T, stats


def pose_error(T, lw_prev, lw_true):
    """(degrees, metres) between the tracked camera T^-1 lw_prev and the true one."""
    lw = track_np.compose(track_np.invert_rigid(T), lw_prev)
    d = track_np.compose(lw, track_np.invert_rigid(lw_true))
    c = min(1.0, max(-1.0, (np.trace(d[:, :3]) - 1.0) / 2.0))
    return math.degrees(math.acos(c)), float(np.linalg.norm(d[:, 3]))
