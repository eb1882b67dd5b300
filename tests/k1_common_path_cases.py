"""Fixtures for the parts of K1's per-pack walk (view_pack, csrc/dfh_integrate.hip) that only few voxels need -- the near-surface
value behind its branch, the singular-pack guard band, the wave-uniform exit of a brick outside the frustum -- on grids of a few
4 x 2 x 32 bricks (tests/test_k1_common_path_fixtures.py on the CPU, tests/test_gpu_k1_common_path.py on the GPU).

classes() counts, from the oracle's chain alone (k1_boundary_cases.chain), how many bricks / packs / voxels of each class a case
holds; a case names the classes it is there for and both tests assert them non-zero.  Nothing here is a golden file."""
import numpy as np

import k1_boundary_cases as B

BRICK = (4, 2, 32)                       # kBrX, kBrY, kBrZ: a wave's 64 lanes hold the brick's 64 z-packs of 4 voxels
GRIDS = {"2x2x2": (8, 4, 64), "ragged": (6, 3, 40)}
BAND_PX = 8 * 2.0 ** -20                 # the guard band round multiples of half a pixel (kFixBand)
WIDE_PX = 2.0 ** -12                     # "certainly not in the band": every fixture keeps non-band voxels this far out


def bricks(a, fill):
    """(X, Y, Z) -> (brick x, brick y, brick z, x, y, z-pack, j), padded with `fill` to whole bricks."""
    nb = [-(-n // b) for n, b in zip(a.shape, BRICK)]
    p = np.full([n * b for n, b in zip(nb, BRICK)], fill, dtype=a.dtype)
    p[:a.shape[0], :a.shape[1], :a.shape[2]] = a
    return p.reshape(nb[0], 4, nb[1], 2, nb[2], 8, 4).transpose(0, 2, 4, 1, 3, 5, 6)


def per_brick(a):
    """Voxel flags (brick..., x, y, z-pack, j) -> per brick: voxels set, lanes (packs) with one set."""
    return a.sum(axis=(3, 4, 5, 6)), a.any(axis=6).sum(axis=(3, 4, 5))


def view_flags(c, lw, dm):
    """Per-voxel classes of one view from the oracle's chain, in brick layout."""
    q = B.chain(dict(c, lw=lw, dm=dm))
    H, W = dm.shape
    u, v = q["u"], q["v"]
    with np.errstate(invalid="ignore", over="ignore"):
        dist = np.minimum(np.abs(2 * u - np.rint(2 * u)), np.abs(2 * v - np.rint(2 * v))) / 2     # px to a multiple of 0.5 px
        in_u, in_v = (u >= 0) & (u <= W - 1), (v >= 0) & (v <= H - 1)
        on_edge = q["ok"] & ~q["vis"] & (((u == W - 1) & in_v) | ((v == H - 1) & in_u))           # outside by the strict <
    band = q["ok"] & (dist <= BAND_PX)
    unsure = q["ok"] & (dist > BAND_PX) & (dist <= WIDE_PX)
    near = q["upd"] & (q["sd"] <= c["tdist"])                     # -tdist < sd <= tdist: the value is sd, not tdist
    sd_tie = q["val"] & (q["sd"] == -c["tdist"])
    f = dict(inside=bricks(np.ones(q["vis"].shape, dtype=bool), False), vis=bricks(q["vis"], False), band=bricks(band, False), unsure=bricks(unsure, False),
             on_edge=bricks(on_edge, False), near=bricks(near, False), sd_tie=bricks(sd_tie, False), upd=bricks(q["upd"], False))
    p2 = bricks(q["p2"], 1.0)
    a, b = p2[..., 0], p2[..., 3]
    f["singular"] = ~((np.abs(a) > 1e-6) & (np.abs(b) > 1e-6) & ((a > 0) == (b > 0))) & f["inside"][..., 0]      # per pack
    return f


def classes(c):
    """Counts over the views of a case (bricks unless said otherwise)."""
    out = dict.fromkeys(("near_only_j0", "near_only_j1", "near_only_j2", "near_only_j3", "near_none", "near_every_lane", "near_one_voxel",
                         "column_none_every_one", "packs_redo_and_near", "packs_singular_between_regular", "singular_brick_outside",
                         "bricks_outside", "bricks_one_voxel_inside", "bricks_edge_band_only", "unsure_voxels"), 0)
    col = {}
    for lw, dm in c["views"]:
        f = view_flags(c, lw, dm)
        out["unsure_voxels"] += int(f["unsure"].sum())
        lanes_in = f["inside"].any(axis=6).sum(axis=(3, 4, 5))
        n_near, l_near = per_brick(f["near"])
        for j in range(4):
            only_j = (n_near > 0) & (f["near"][..., j].sum(axis=(3, 4, 5)) == n_near)
            out["near_only_j%d" % j] += int(only_j.sum())
        swept = f["vis"].any(axis=(3, 4, 5, 6))                    # bricks the view reaches at all
        none, every, one = swept & (n_near == 0), (l_near == lanes_in) & (lanes_in > 0), n_near == 1
        out["near_none"] += int(none.sum())
        out["near_every_lane"] += int(every.sum())
        out["near_one_voxel"] += int(one.sum())
        for key, m in (("none", none), ("every", every), ("one", one)):
            col[key] = col.get(key, False) | m.any(axis=2)
        # a guard-band voxel (re-run exactly) and a plain near-surface voxel in ONE pack
        redo = (f["vis"] & f["band"]) | f["sd_tie"]
        plain = f["near"] & ~f["band"] & ~f["unsure"] & ~f["sd_tie"]
        out["packs_redo_and_near"] += int((redo.any(axis=6) & plain.any(axis=6) & ~f["singular"]).sum())
        # singular packs with regular neighbours along z in their lane row
        s = f["singular"]
        reg = ~s & f["inside"][..., 0]
        between = s.copy()
        between[..., 1:] &= reg[..., :-1]
        between[..., :-1] &= reg[..., 1:]
        out["packs_singular_between_regular"] += int(between.sum())
        cand = f["vis"] | f["band"] | f["unsure"]
        cand_reg = (cand & ~s[..., None]).any(axis=(3, 4, 5, 6))
        out["singular_brick_outside"] += int((s.any(axis=(3, 4, 5)) & ~cand_reg).sum())
        any_s = s.any(axis=(3, 4, 5))
        n_vis, _ = per_brick(f["vis"])
        out["bricks_outside"] += int((~cand.any(axis=(3, 4, 5, 6)) & ~any_s).sum())
        out["bricks_one_voxel_inside"] += int(((n_vis == 1) & ~any_s).sum())
        out["bricks_edge_band_only"] += int(((n_vis == 0) & ~any_s & f["on_edge"].any(axis=(3, 4, 5, 6))).sum())
    out["column_none_every_one"] = int((col["none"] & col["every"] & col["one"]).sum())
    return out


# ------------------------------------------------------------------------------------------------------------------ the cases
SCALE, TSDF_RES = 0.125, 8               # voxel (ix, iy, iz) at 0.125 (i - 4): dyadic, as in k1_boundary_cases


def _lw(t, angle_deg=0.0, eye=None):
    """World -> camera: the identity rotation with translation t, or a rotation about y with the camera centre at `eye`."""
    if eye is None:
        return np.concatenate([np.eye(3), np.asarray(t, dtype=np.float64).reshape(3, 1)], axis=1)
    a = np.radians(angle_deg)
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    return np.concatenate([R, (-R @ np.asarray(eye, dtype=np.float64))[:, None]], axis=1)


def _case(name, grid, K, tdist, views, claims, margin_zero=False):
    Km, Kinv = K
    return dict(name="%s-%s" % (name, grid), res=GRIDS[grid], tsdf_res=TSDF_RES, scale=SCALE, center=np.zeros(3), tdist=tdist, K=Km,
                Kinv=Kinv, views=views, claims=claims, margin_zero=margin_zero)


def _wall(hw, layer, tz):
    """A flat wall through the voxel centres of z layer `layer` (sd == 0 there) for a camera at z translation tz."""
    return np.full(hw, -(SCALE * (layer - TSDF_RES / 2) + tz))


def _cases(grid):
    out = []
    front = _lw((0, 0, 2.0))
    K_off = B.dyadic_K(64.0, 64.0, 24.25, 24.25)              # principal point off the half-pixel lattice: the whole grid in view
    # 1. tdist = half a voxel: exactly one z layer is near the surface -- layer 36 + j of the bricks bz = 1 (view 0), layer 8 + j of
    #    the bricks bz = 0 (view 1, shifted sideways)
    for j in range(4):
        views = [(front, _wall((48, 64), 36 + j, 2.0)), (_lw((0.0625, 0, 2.0)), _wall((48, 64), 8 + j, 2.0))]
        out.append(_case("wall_j%d" % j, grid, K_off, SCALE / 2, views, ("near_only_j%d" % j,)))
    # 2. an oblique wall (depth linear in the pixel) and tdist = 20 voxels: the band takes in the whole of the bricks bz = 1 and
    #    cuts one corner voxel off a brick bz = 0; view 1: a wall far behind the grid (every voxel it updates is in free space)
    uu, vv = np.meshgrid(np.arange(64.0), np.arange(48.0))
    oblique = -(7.90625 + (uu - 24.25) / 32 + (vv - 24.25) / 64)
    far = np.full((48, 64), -40.0)
    far[::5, ::7] = 0.0                                         # (some pixels without depth: not every voxel is updated)
    out.append(_case("oblique", grid, K_off, 2.5, [(front, oblique), (front, far)],
                     ("near_none", "near_every_lane", "near_one_voxel", "column_none_every_one")))
    # 3. exact arithmetic, margin 0: tdist = two voxels, the wall through layer 33 / 9 -- layer + 2 has sd == -tdist exactly
    #    (re-run exactly, not updated) in one pack with the near-surface layers below it; the principal point on a half pixel puts
    #    u on a tie along x = 4 as well
    K_half = B.dyadic_K(64.0, 64.0, 24.5, 24.0)
    out.append(_case("redo_and_near", grid, K_half, 2 * SCALE, [(front, _wall((48, 64), 33, 2.0)), (front, _wall((48, 64), 9, 2.0))],
                     ("packs_redo_and_near",), margin_zero=True))
    # 4. the camera inside the grid, turned 45 degrees about y: its plane crosses the z rows one pack further per voxel in x, so
    #    single lanes hold singular packs; the tall narrow image leaves the bricks of the rows y >= 2 outside the frustum
    eye = (-0.47, -0.47, 1.0)
    lw_in = _lw(None, -45.0, eye)
    lw_in2 = lw_in.copy()
    lw_in2[2, 3] += 0.26
    dm = np.full((48, 64), -2.0)
    dm[::3, ::4] = 0.0
    out.append(_case("camera_plane", grid, B.dyadic_K(256.0, 512.0, 32.25, 24.25), 2 * SCALE, [(lw_in, dm), (lw_in2, dm)],
                     ("packs_singular_between_regular", "singular_brick_outside")))
    # 5. narrow frustums.  View 0: l2 = odd / 32, no voxel anywhere near a tie -- bricks wholly outside, bricks with one voxel
    #    inside.  View 1: u == W - 1 exactly (outside, by the strict <) on the voxels (4, y, 31) of bricks that are otherwise outside
    (W_, H_), (tx, ty) = {"2x2x2": ((16, 12), (-36 / 64, 52 / 64)), "ragged": ((8, 8), (-19 / 64, 6 / 64))}[grid]
    narrow = (B.dyadic_K(64.0, 64.0, W_ / 2 + 0.25, H_ / 2 + 0.25), _lw((tx, ty, 2.03125)), np.full((H_, W_), -5.0))
    edge = (B.dyadic_K(64.0, 64.0, 5.0, 24.0), _lw((43 / 256, 0.5, 2.0)), np.full((48, 8), -5.0))
    for name, (K, lw, dm), claims in (("narrow", narrow, ("bricks_outside", "bricks_one_voxel_inside")), ("edge", edge, ("bricks_edge_band_only",))):
        out.append(_case(name, grid, K, 2 * SCALE, [(lw, dm), (lw, dm)], claims))
    return out


CASES = [c for grid in GRIDS for c in _cases(grid)]
