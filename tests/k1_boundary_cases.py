"""Fixtures for K1 at its decision boundaries (tests/test_k1_boundary_fixtures.py on the CPU, tests/test_gpu_k1_boundaries.py on
the GPU): cameras for which every fp64 operation of fuseDepths' chain (core/fusion_dm.py:191-203) is EXACT, so that the
reference's answer at a tie does not depend on the summation order of its BLAS and a margin of exactly 0 is legitimate.

  * lw is the identity rotation with a dyadic translation; scale, centre, tdist, K and every depth are dyadic with few bits:
    index -> pos -> lpos -> K lpos are sums and products of small dyadic numbers, all exact in fp64;
  * u = p0 / p2 and v = p1 / p2 are single IEEE divisions of exact operands: correctly rounded, whatever the order of the sums;
  * K^-1 is written down in closed form (dyadic; its last row is exactly (0, 0, 1)), not taken from a linear solver.

voxel_classes() counts, from the oracle's side alone, the voxels of each boundary class; a case names the classes it is there
for and the tests assert that each holds at least MIN_CLASS voxels (a later change of a fixture cannot move off the boundaries
without a failure).  Nothing here is a golden file: everything is generated from the constants below."""
import numpy as np

MIN_CLASS = 10


def dyadic_K(fx, fy, cx, cy, skew=0.0):
    """(K, K^-1) of an upper-triangular camera matrix with power-of-two focal lengths: the inverse in closed form, exact."""
    K = np.array([[fx, skew, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    Kinv = np.array([[1.0 / fx, -skew / (fx * fy), (skew * cy - cx * fy) / (fx * fy)], [0.0, 1.0 / fy, -cy / fy], [0.0, 0.0, 1.0]])
    assert np.array_equal(K @ Kinv, np.eye(3)) and np.array_equal(Kinv @ K, np.eye(3))
    return K, Kinv


def striped_depth(H, W, far=-4.5, near=-2.5):
    """A wall at `far`, pixels [::3, ::4] without depth, rows 1::5 at `near` (in that order)."""
    dm = np.full((H, W), far)
    dm[::3, ::4] = 0.0
    dm[1::5] = near
    return dm


def _case(name, res, tsdf_res, scale, tdist, hw, K, t, claims, dm=None, center=(0.0, 0.0, 0.0)):
    Km, Kinv = K
    lw = np.concatenate([np.eye(3), np.asarray(t, dtype=np.float64).reshape(3, 1)], axis=1)
    return dict(name=name, res=res, tsdf_res=tsdf_res, scale=scale, center=np.asarray(center, dtype=np.float64), tdist=tdist,
                K=Km, Kinv=Kinv, lw=lw, dm=striped_depth(*hw) if dm is None else dm, claims=claims)


ALL = ("tie", "edge", "no_depth", "sd_tie")
EXACT_CASES = [
    # the camera in front of a 16 x 16 x 32 grid of pitch 1/4: principal point on a half pixel in u / in v
    _case("front", (16, 16, 32), 16, 0.25, 0.5, (25, 34), dyadic_K(32.0, 32.0, 16.5, 12.0), (0, 0, 5), ALL),
    _case("swap", (16, 16, 32), 16, 0.25, 0.5, (25, 34), dyadic_K(32.0, 32.0, 16.0, 12.5), (0, 0, 5), ALL),
    # the camera inside the grid, its plane through voxel centres: p2 == 0, voxels behind the camera that are updated
    _case("inside", (16, 16, 32), 16, 0.25, 0.5, (25, 34), dyadic_K(32.0, 32.0, 16.5, 12.0), (0, 0, -1), ALL + ("p2_zero", "behind")),
    # general 3 x 3 path: skew, fy != fx
    _case("skew", (16, 16, 32), 16, 0.25, 0.5, (41, 38), dyadic_K(32.0, 64.0, 16.5, 20.0, skew=4.0), (0, 0, 5), ALL),
    _case("skew_inside", (16, 16, 32), 16, 0.25, 0.5, (41, 38), dyadic_K(32.0, 64.0, 16.5, 20.0, skew=4.0), (0, 0, -1),
          ALL + ("p2_zero", "behind")),
    # ragged Z (VEC = 1)
    _case("ragged", (16, 16, 30), 16, 0.25, 0.5, (25, 34), dyadic_K(32.0, 32.0, 16.5, 12.0), (0, 0, 5), ALL),
    # five 4 x 2 x 32 bricks along z, most of them behind the wall or outside the frustum: the column walk and the culling passes act
    _case("bricks", (24, 20, 160), 24, 0.125, 0.5, (50, 70), dyadic_K(64.0, 64.0, 34.5, 24.0), (0, 0, 1.75), ALL),
    _case("bricks_inside", (24, 20, 160), 24, 0.125, 0.5, (50, 70), dyadic_K(64.0, 64.0, 34.5, 24.0), (0, 0, -0.5),
          ALL + ("p2_zero", "behind")),
]


def chain(c, dm=None):
    """The oracle's per-voxel quantities for a case, in its own operation order (oracle_np.fuse_depths)."""
    dm = c["dm"] if dm is None else dm
    H, W = dm.shape
    X, Y, Z = c["res"]
    K, Kinv, lw, scale, center, half = c["K"], c["Kinv"], c["lw"], c["scale"], c["center"], c["tsdf_res"] / 2
    ix = np.arange(X, dtype=np.float32).astype(np.float64)[:, None, None]
    iy = np.arange(Y, dtype=np.float32).astype(np.float64)[None, :, None]
    iz = np.arange(Z, dtype=np.float32).astype(np.float64)[None, None, :]
    px = scale * (ix - half) + center[0]
    py = scale * (iy - half) + center[1]
    pz = scale * (iz - half) + center[2]
    l0 = lw[0, 0] * px + lw[0, 1] * py + lw[0, 2] * pz + lw[0, 3]
    l1 = lw[1, 0] * px + lw[1, 1] * py + lw[1, 2] * pz + lw[1, 3]
    l2 = lw[2, 0] * px + lw[2, 1] * py + lw[2, 2] * pz + lw[2, 3]
    p0 = K[0, 0] * l0 + K[0, 1] * l1 + K[0, 2] * l2
    p1 = K[1, 0] * l0 + K[1, 1] * l1 + K[1, 2] * l2
    p2 = K[2, 0] * l0 + K[2, 1] * l1 + K[2, 2] * l2
    ok = p2 != 0
    p2s = np.where(ok, p2, 1.0)
    u, v = p0 / p2s, p1 / p2s
    vis = ok & (u >= 0) & (u < W - 1) & (v >= 0) & (v < H - 1)
    ui = np.where(vis, np.rint(u), 0).astype(np.int64)
    vi = np.where(vis, np.rint(v), 0).astype(np.int64)
    z = -1 * dm[vi, ui].astype(np.float64)
    val = vis & (z > 0)
    with np.errstate(invalid="ignore", over="ignore"):
        cz = Kinv[2, 0] * (z * u) + Kinv[2, 1] * (z * v) + Kinv[2, 2] * (z * 1.0)
        sd = cz - l2
        upd = val & (sd > -1 * c["tdist"])
    return dict(u=u, v=v, ok=ok, vis=vis, ui=ui, vi=vi, z=z, val=val, sd=sd, upd=upd, l2=l2, p2=p2 + 0 * u)


def voxel_classes(c, dm=None):
    """Voxel counts of the boundary classes of a case, from the oracle's chain:
       tie      a visible voxel with u or v exactly on .5 (round half to even decides the pixel);
       edge     u or v exactly 0 (inside, >=) or exactly W - 1 / H - 1 (outside, strict <), the other coordinate in range;
       p2_zero  on the camera plane (never projected);
       no_depth visible, its pixel holds z == 0 (strict z > 0);
       sd_tie   a valid pixel and sd == -tdist exactly (strict >: not updated);
       behind   updated although lpos_z < 0 (the reference never tests it)."""
    q = chain(c, dm)
    H, W = (c["dm"] if dm is None else dm).shape
    u, v = q["u"], q["v"]
    in_u, in_v = (u >= 0) & (u <= W - 1), (v >= 0) & (v <= H - 1)
    return dict(tie=int((q["vis"] & ((u - np.floor(u) == 0.5) | (v - np.floor(v) == 0.5))).sum()),
                edge=int((q["ok"] & ((((u == 0) | (u == W - 1)) & in_v) | (((v == 0) | (v == H - 1)) & in_u))).sum()),
                p2_zero=int((~q["ok"]).sum()),
                no_depth=int((q["vis"] & (q["z"] == 0)).sum()),
                sd_tie=int((q["val"] & (q["sd"] == -c["tdist"])).sum()),
                behind=int((q["upd"] & (q["l2"] < 0)).sum()),
                updated=int(q["upd"].sum()))
