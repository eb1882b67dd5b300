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


# ---- maps with more tiles than the rows kernel has workgroups -------------------------------------------------------------------
# icp_rows_kernel runs ICP_GRID workgroups per view; workgroup b walks the 16 x 16-pixel tiles b, b + ICP_GRID, ...  A "pass" p is
# the tiles 256 p .. 256 p + 255 that exist: what the grid does in one turn of that loop.  The shapes are chosen by tile count.
ICP_GRID = 256
PASS_SHAPES = {                         # (H, W): (tiles, passes)
    (16, 4080): (255, 1),               # one below the grid
    (16, 4096): (256, 1),               # exactly the grid
    (16, 4112): (257, 2),               # one workgroup takes two tiles
    (16, 8208): (513, 3),               # one workgroup takes three tiles
    (272, 272): (289, 2),               # two-dimensional, full tiles
    (257, 528): (561, 3),               # 2 * 256 + 49: a partial third pass whose last tile row is one pixel high
}
PASS_GATES = dict(max_dist=0.1, min_cos=0.8, huber=0.01)
NO_MEASUREMENT = (np.nan, np.inf, -np.inf, -0.0, 0.0, 2.5)     # the classes of tests/test_gpu_track.special_depth


def n_tiles(h, w):
    return ((w + 15) // 16) * ((h + 15) // 16)


def tile_index(h, w):
    """(h, w) int: the index of the 16 x 16 tile a pixel lies in, row-major over tiles (the kernel's tile -> pixel map, inverted)."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return (y // 16) * ((w + 15) // 16) + x // 16


def pass_intrinsics(h, w):
    return np.array([[0.9 * w, 0.0, (w - 1) / 2.0], [0.0, 0.9 * w, (h - 1) / 2.0], [0.0, 0.0, 1.0]])


def sprinkle(rng, depth, normals):
    """Every class of 'no measurement', and pixels without a normal, over a diagonal band that crosses every tile (in place)."""
    h, w = depth.shape
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    band = (x + 3 * y) % 16 < 3
    pick = rng.random((h, w))
    for k, v in enumerate(NO_MEASUREMENT):
        depth[band & (pick >= 0.04 * k) & (pick < 0.04 * (k + 1))] = v
    normals[band & (rng.random((h, w)) < 0.1)] = 0.0


_PASS_CASES = {}


def pass_case(h, w):
    """The scene through pass_intrinsics(h, w): the model from the identity, the live map from motion(0.3), both sprinkled; two
    views of the same maps with different T (the identity; a small twist); the restatement's rows under
    PASS_GATES.  Built once per shape and shared, CPU and GPU tests alike: nobody writes to it."""
    if (h, w) not in _PASS_CASES:
        Kp = pass_intrinsics(h, w)
        rng = np.random.default_rng(1000 * h + w)
        md, mn = render(IDENT, Kp, h, w)
        ld, ln = render(motion(0.3), Kp, h, w)
        sprinkle(rng, md, mn)
        sprinkle(rng, ld, ln)
        # (a 16-row map through f = 0.9 w: a prior that moved the projection by more than a few rows would leave no row at all;
        # the second view's turns about y and moves along x and z, which shift it along the rows, inwards at the last tile)
        Ts = np.stack([IDENT, track_np.apply_twist(np.array([2e-4, -4e-3, 1e-3, -0.01, 2e-4, 0.005]), IDENT)])
        Dl, Nl, Dm, Nm = np.stack([ld, ld]), np.stack([ln, ln]), np.stack([md, md]), np.stack([mn, mn])
        rows = np.stack([track_np.icp_rows(Dl[v], Nl[v], Dm[v], Nm[v], Kp, np.linalg.inv(Kp), Ts[v], **PASS_GATES) for v in range(2)])
        for a in (Dl, Nl, Dm, Nm, Ts, rows):
            a.setflags(write=False)
        _PASS_CASES[(h, w)] = dict(K=Kp, Dl=Dl, Nl=Nl, Dm=Dm, Nm=Nm, Ts=Ts, rows=rows, tile=tile_index(h, w))
    return _PASS_CASES[(h, w)]


def pose_error(T, lw_prev, lw_true):
    """(degrees, metres) between the tracked camera T^-1 lw_prev and the true one."""
    lw = track_np.compose(track_np.invert_rigid(T), lw_prev)
    d = track_np.compose(lw, track_np.invert_rigid(lw_true))
    c = min(1.0, max(-1.0, (np.trace(d[:, :3]) - 1.0) / 2.0))
    return math.degrees(math.acos(c)), float(np.linalg.norm(d[:, 3]))
