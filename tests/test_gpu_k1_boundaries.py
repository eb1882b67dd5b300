"""K1 (depth map -> TSDF) and the projective association driven onto their decision boundaries and over bad depth values, on
every sweep K1 has, against the fp64 oracles (oracle/oracle_np.py, oracle/oracle_c.c).

The bars are the project's own, no new tolerance: masks and weights array_equal, float64 volumes
array_equal, float32 values |dT| <= 2 n eps32 (1 + |T|) after n integrations, and every float32 sweep gives every other's
volumes bit for bit.

  a. exact-arithmetic cameras (tests/k1_boundary_cases.py): voxels exactly on .5-pixel ties, on the frustum's edges, on the
     camera plane, on pixels without depth, on sd == -tdist, and behind the camera -- margin exactly 0, class counts asserted;
  b. depths nudged -4 .. +4 ulp across sd == -tdist on an ordinary camera, in metre- and millimetre-like units;
  c. NaN, +-inf, wrong sign, +-0, -FLT_MAX, subnormal and (float64 maps) out-of-float32-range depths scattered over a map;
  d. depth maps 2048 and 2049 pixels wide / high: the fast path's last size and the exact path's first;
  e. the association (dfh_gn_associate, the fused dfh_gn_build) on frames that carry the bad values of c."""
import numpy as np
import pytest
import torch

import k1_boundary_cases as B
from oracle import gn_np as G
from oracle import oracle_c as OC
from oracle import oracle_np as O
from dynamicfusion_body_amd import FusionDM, _lib, kernels, scene
from dynamicfusion_body_amd.pipeline import FrameSolver

pytestmark = pytest.mark.gpu

F32_EPS = float(np.finfo(np.float32).eps)
F32_TINY = float(np.finfo(np.float32).tiny)               # smallest normal
F32_SUB = float(np.float32(1e-45))                         # smallest subnormal, 2^-149
F32_MAX = float(np.finfo(np.float32).max)

K1_OPTIONS = ("k1_no_bricks", "k1_bricks_min", "k1_cull", "k1_gather_first", "k1_nzi", "k1_late_loads", "k1_force_scalar", "k1_prefetch")
COLUMNS = {"k1_bricks_min": 0, "k1_nzi": 16}
# name -> (options, how): "single" = one dfh_integrate_depth per view, "multi" = one dfh_integrate_depth for all the views, "fresh" = its fresh
# variant, "f64" = a float64 volume (the exact kernel).  Grids whose Z is no multiple of 4 (and k1_force_scalar) take VEC = 1
# instances of the row and multi-view sweeps; they have no column walk and fall back to rows.
SWEEPS = {
    "rows": ({"k1_no_bricks": 1, "k1_late_loads": 1}, "single"),
    "rows_early": ({"k1_no_bricks": 1}, "single"),                          # slabs up to 2^23 voxels: the early-load row sweep
    "rows_vec1": ({"k1_no_bricks": 1, "k1_force_scalar": 1}, "single"),
    "columns": (dict(COLUMNS, k1_cull=0, k1_gather_first=0), "single"),
    "columns_prefetch": (dict(COLUMNS, k1_cull=0, k1_gather_first=0, k1_prefetch=1), "single"),
    "columns_culled": (dict(COLUMNS, k1_cull=1, k1_gather_first=0), "single"),     # depth pyramid + classification pass
    "gather_first": (dict(COLUMNS, k1_cull=0, k1_gather_first=1), "single"),
    "gather_first_culled": (dict(COLUMNS, k1_cull=1, k1_gather_first=1), "single"),
    "gather_first_one_brick": (dict(COLUMNS, k1_cull=0, k1_gather_first=1, k1_nzi=1), "single"),
    "multi_columns_culled": ({}, "multi"),
    "multi_columns": ({"k1_bricks_nocull": 1}, "multi"),
    "multi_rows": ({"k1_no_bricks": 1}, "multi"),
    "multi_rows_vec1": ({"k1_no_bricks": 1, "k1_force_scalar": 1}, "multi"),
    "fresh_columns": ({}, "fresh"),
    "fresh_rows": ({"k1_no_bricks": 1}, "fresh"),
    "exact_f64": ({}, "f64"),
    "exact_f64_vec1": ({"k1_force_scalar": 1}, "f64"),
}


def set_options(opts):
    for name in K1_OPTIONS + ("k1_bricks_nocull",):
        _lib.set_option(name, opts.get(name))


def run_sweep(name, res, tsdf_res, K, Kinv, scale, center, tdist, wmax, views, ddt):
    """The volumes (from T = tdist, w = 0) after `views` = [(lw, depth map as numpy)] on sweep `name`."""
    opts, how = SWEEPS[name]
    vdt = torch.float64 if how == "f64" else torch.float32
    T = torch.full(res, tdist, dtype=vdt, device="cuda")
    Wt = torch.zeros_like(T)
    with np.errstate(over="ignore"):
        ds = [torch.from_numpy(np.ascontiguousarray(dm)).to("cuda", dtype=ddt).contiguous() for _, dm in views]
    lws = [lw for lw, _ in views]
    set_options(opts)
    try:
        if how in ("single", "f64"):
            for lw, d in zip(lws, ds):
                kernels.integrate_depth(T, Wt, d, K, Kinv, lw, scale, center, tdist, wmax, tsdf_res=tsdf_res)
        else:
            # one view would be handed to the single-view sweeps (dfh_integrate_depth: n_views == 1): every case passes two or more
            assert len(views) >= 2, "the multi-view sweeps need at least two views"
            if how == "fresh":
                T.fill_(float("nan")); Wt.fill_(7.0)                                   # garbage: the sweep writes every voxel
            H, W_ = ds[0].shape
            ws = kernels.integrate_workspace(len(ds), H, W_, res, None, T.device)        # (the cached one the call below uses)
            ws.zero_()
            kernels.integrate_depth_views(T, Wt, ds, K, Kinv, lws, scale, center, tdist, wmax, tsdf_res=tsdf_res,
                                          fresh=tdist if how == "fresh" else None)
            torch.cuda.synchronize()
            if max(H, W_) <= 2048:
                # the multi-view kernels ran, not one single-view sweep per view: the views' parameter records are the first
                # region of the workspace and only the multi-view path uploads them (record 1 holds view 1's K: non-zero) ...
                rec = kernels.integrate_workspace_params_doubles(ws, len(ds))
                assert bool((rec[1] != 0).any()), "%s: the multi-view path was not taken" % name
                # ... and behind the culling passes the classification wrote a bit for view 1 into some brick's mask
                if name in ("multi_columns_culled", "fresh_columns") and res[2] % 4 == 0:
                    assert bool(((kernels.brick_masks(ws, res).int() & 0xFFFF) >> 1).any()), "%s: no brick mask names a second view" % name
        torch.cuda.synchronize()
    finally:
        set_options({})
    return T, Wt


def oracle_volumes(res, tsdf_res, K, Kinv, scale, center, tdist, wmax, views, ddt):
    """numpy oracle and C oracle on the depth values the device sees (the map rounded to its type): the same volumes bit for bit."""
    kw = dict(tsdf_res=tsdf_res, scale=scale, center=center, wmax=wmax)
    Tn, Wn = np.zeros(res) + tdist, np.zeros(res)
    Tc, Wc = Tn.copy(), Wn.copy()
    masks, margin = [], [None]
    for lw, dm in views:
        with np.errstate(all="ignore"):
            d = dm.astype(np.float32) if ddt == torch.float32 else dm.astype(np.float64)
            _, _, m = O.fuse_depths(d, lw, K, Kinv, Tn, Wn, tdist, return_mask=True, margin_out=margin, **kw)
        OC.fuse_depths(d, lw, K, Kinv, Tc, Wc, tdist, **kw)
        masks.append(m)
    assert np.array_equal(Wn, Wc) and np.array_equal(Tn, Tc), "the two oracles disagree"
    assert np.isfinite(Tn).all() and np.isfinite(Wn).all()
    return Tn, Wn, masks, margin[0]


def check_all_sweeps(res, tsdf_res, K, Kinv, scale, center, tdist, wmax, views, ddt):
    """Every sweep against the oracle and against each other; returns the oracle's (T, w, per-view masks, margin)."""
    OC.build()
    To, Wo, masks, margin = oracle_volumes(res, tsdf_res, K, Kinv, scale, center, tdist, wmax, views, ddt)
    n = len(views)
    first = None
    for name in SWEEPS:
        T, Wt = run_sweep(name, res, tsdf_res, K, Kinv, scale, center, tdist, wmax, views, ddt)
        Tg, Wg = T.cpu().numpy().astype(np.float64), Wt.cpu().numpy().astype(np.float64)
        assert np.isfinite(Tg).all() and np.isfinite(Wg).all(), "%s: NaN or Inf in T / w" % name
        bad = int((Wg != Wo).sum())
        assert bad == 0, "%s: mask / weights differ from the oracle on %d voxels, e.g. %s" % (name, bad, np.argwhere(Wg != Wo)[:4].tolist())
        if T.dtype == torch.float64:
            assert np.array_equal(Tg, To), "%s: float64 T differs from the oracle" % name
            continue
        err = np.abs(Tg - To) / (1 + np.abs(To))
        assert err.max() <= 2.0 * n * F32_EPS, "%s: |dT| / (1 + |T|) = %.3g" % (name, err.max())
        if first is None:
            first = (name, T, Wt)
        else:
            assert torch.equal(T, first[1]) and torch.equal(Wt, first[2]), "%s and %s differ" % (name, first[0])
    return To, Wo, masks, margin


# --------------------------------------------------------------------------------------------------------- a. exact cameras
@pytest.mark.parametrize("ddt", [torch.float32, torch.float64], ids=["f32map", "f64map"])
@pytest.mark.parametrize("case", B.EXACT_CASES, ids=[c["name"] for c in B.EXACT_CASES])
def test_exact_arithmetic_cameras_at_margin_zero(case, ddt):
    """Voxels exactly ON every decision boundary (class counts from the oracle's side, asserted; the oracle's margin is exactly
    0): the same view twice, every sweep.  Counts reached (voxels per class): tests/k1_boundary_cases.py and DESIGN.md section 4."""
    c = case
    counts = B.voxel_classes(c)
    print("exact case %s: %s" % (c["name"], counts))
    for name in c["claims"]:
        assert counts[name] >= B.MIN_CLASS, (name, counts)
    views = [(c["lw"], c["dm"]), (c["lw"], c["dm"])]
    To, Wo, masks, margin = check_all_sweeps(c["res"], c["tsdf_res"], c["K"], c["Kinv"], c["scale"], c["center"], c["tdist"], 3.0, views, ddt)
    assert margin == 0.0
    assert int(masks[0].sum()) == counts["updated"] and 0 < counts["updated"] < Wo.size


# ------------------------------------------------------------------------------------------- b. depths nudged across sd = -tdist
def _ordinary_camera(pinhole, units):
    """A scene.py camera (prime-numerator intrinsics, rotated view) on a 32^3 grid; units = 1 (metres) or 1000 (millimetre-like
    world coordinates: scale, centre, tdist, the extrinsic's translation and the depths all 1000 times larger)."""
    R, (H, W_) = 32, (60, 80)
    fx = 0.93 * W_ + 0.137
    K = scene.intrinsics(fx, W_ / 2 - 0.2713, H / 2 + 0.1371)
    if not pinhole:
        K[0, 1] = 0.31
        K[1, 1] = fx * 1.07
    lw = scene.view_extrinsic(20.0)
    dm = scene.render_depth(K, lw, H, W_, invalid_frac=0.03, seed=11) * units
    lw = lw.copy()
    lw[:, 3] *= units
    scale, center, tdist = scene.grid_params(R)
    return dict(res=(R, R, R), tsdf_res=R, K=K, Kinv=np.linalg.inv(K), lw=lw, scale=scale * units, center=center * units,
                tdist=tdist * units, dm=dm)


def _ulp_step(a, k):
    """a (positive, float32 or float64) moved by k units in the last place of its own type."""
    bits = a.view(np.int32 if a.dtype == np.float32 else np.int64)
    return (bits + k).view(a.dtype)


@pytest.mark.parametrize("ddt", [torch.float32, torch.float64], ids=["f32map", "f64map"])
@pytest.mark.parametrize("units", [1.0, 1000.0], ids=["metres", "millimetres"])
@pytest.mark.parametrize("pinhole", [True, False], ids=["pinhole", "skewed"])
def test_depths_nudged_across_the_truncation_boundary(pinhole, units, ddt):
    """Per picked voxel (visible, valid pixel, one voxel per pixel) the depth at which sd == -tdist, computed in the oracle's
    fp64 order, moved by -4 .. +4 ulp of the map's type and stored in its pixel: the oracle decides, the masks are bit-exact.
    At 1000-fold coordinates |l2| ~ 1.5e3 .. 2.5e3 and float32 rounding of l2 / z (1e-4) is ten times the band's constant term:
    the 2e-6 |l2| term is what keeps the float32 decision honest.  Counts reached: see DESIGN.md section 4."""
    c = _ordinary_camera(pinhole, units)
    npdt = np.float32 if ddt == torch.float32 else np.float64
    q = B.chain(c)
    cand = q["val"] & (q["l2"] > 2.0 * c["tdist"])
    flat = np.flatnonzero(cand)
    pix = (q["vi"] * c["dm"].shape[1] + q["ui"]).reshape(-1)[flat]
    rng = np.random.default_rng(3)
    order = rng.permutation(flat.size)
    _, first = np.unique(pix[order], return_index=True)            # one voxel per pixel, a random one
    picked = flat[order[first]]
    picked = picked[rng.permutation(picked.size)[:900]]
    assert picked.size >= 200
    u, v, l2 = (q[name].reshape(-1)[picked] for name in ("u", "v", "l2"))
    Kinv = c["Kinv"]
    # sd = (Kinv[2,0] (z u) + Kinv[2,1] (z v) + Kinv[2,2] z) - l2 == -tdist
    z0 = (l2 - c["tdist"]) / (Kinv[2, 0] * u + Kinv[2, 1] * v + Kinv[2, 2])
    k = (np.arange(picked.size) % 9) - 4
    zk = _ulp_step(z0.astype(npdt), k.astype(np.int32 if npdt == np.float32 else np.int64))
    dm = c["dm"].astype(npdt)
    dm.reshape(-1)[pix_of(q, c, picked)] = -zk
    views = [(c["lw"], dm), (c["lw"], dm)]                         # twice: one view alone never reaches the multi-view kernels
    To, Wo, masks, margin = check_all_sweeps(c["res"], c["tsdf_res"], c["K"], c["Kinv"], c["scale"], c["center"], c["tdist"], 100.0, views, ddt)
    got = masks[0].reshape(-1)[picked]
    n_upd, n_not = int(got.sum()), int((~got).sum())
    sd = B.chain(c, dm)["sd"].reshape(-1)[picked]
    print("nudged %s units=%g %s: %d picked, %d updated, %d not; |sd + tdist| <= %.3g, smallest %.3g"
          % ("pinhole" if pinhole else "skewed", units, npdt.__name__, picked.size, n_upd, n_not, np.abs(sd + c["tdist"]).max(),
             np.abs(sd + c["tdist"]).min()))
    assert n_upd >= 20 and n_not >= 20                              # both outcomes, from the oracle
    # every picked voxel sits within a few ulp of the boundary -- far inside the float32 band 2e-6 |l2| + 1e-5
    assert np.abs(sd + c["tdist"]).max() <= 16 * float(np.finfo(npdt).eps) * np.abs(l2).max()


def pix_of(q, c, picked):
    return (q["vi"] * c["dm"].shape[1] + q["ui"]).reshape(-1)[picked]


# ------------------------------------------------------------------------------------------------------ c. bad depth values
BAD_BOTH = [("nan", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf")), ("positive", 1.25), ("+0", 0.0), ("-0", -0.0),
            ("-FLT_MAX", -F32_MAX), ("-subnormal", -F32_SUB), ("-tiny", -F32_TINY)]
BAD_F64 = [("-1e-50", -1e-50), ("-1e-320", -1e-320), ("-1e39", -1e39), ("-1e300", -1e300), ("-1.5e308", -1.5e308)]
# -inf: the reference forms K^-1 (z [u, v, 1]) with a matrix product, its third row (0, 0, 1) meets z u = inf, 0 * inf = NaN, and a
# NaN sd updates nothing (core/fusion_dm.py:198-203) -- with every K.  -1.5e308 does the same wherever z u or z v overflows
# (u or v above 1.19) and updates elsewhere: the oracle decides voxel by voxel.
NEVER = ("nan", "+inf", "positive", "+0", "-0", "-inf")
FAR = ("-FLT_MAX", "-1e39", "-1e300")
TINY = ("-subnormal", "-tiny", "-1e-50", "-1e-320")


def bad_values(ddt):
    return BAD_BOTH + (BAD_F64 if ddt == torch.float64 else [])


def scatter_bad(dm, hit_pixels, values, rng, frac=0.5):
    """`values` over a random `frac` of the flat pixel indices `hit_pixels`, in turn; returns {name: flat pixel indices}."""
    dm = dm.copy()
    sel = rng.permutation(hit_pixels)[:max(int(frac * hit_pixels.size), 4 * len(values))]
    where = {}
    for i, (name, val) in enumerate(values):
        where[name] = sel[i::len(values)]
        dm.reshape(-1)[where[name]] = val
    return dm, where


def _bad_depth_views(pinhole, ddt, res):
    R = res[0]
    H, W_ = 60, 80
    fx = 0.93 * W_ + 0.137
    K = scene.intrinsics(fx, W_ / 2 - 0.2713, H / 2 + 0.1371)
    if not pinhole:
        K[0, 1] = 0.31
        K[1, 1] = fx * 1.07
    Kinv = np.linalg.inv(K)
    scale, center = scene.GRID_SIDE / R, scene.SPHERE_C.copy()
    tdist = 4.0 * scale
    lw_out = scene.view_extrinsic(-25.0)
    lw_in = scene.view_extrinsic(15.0)
    lw_in[2, 3] -= float(lw_in[2, :3] @ center + lw_in[2, 3]) - 0.013            # the grid's centre 13 mm in front of the camera
    lw_near = scene.view_extrinsic(40.0)
    lw_near[2, 3] -= 1.15                                                        # the camera plane 5 cm in front of the grid's near corner region
    c = dict(res=res, tsdf_res=R, K=K, Kinv=Kinv, scale=scale, center=center, tdist=tdist)
    rng = np.random.default_rng(19)
    views, stats = [], []
    for lw in (lw_out, lw_in, lw_near):
        base = scene.render_depth(K, lw, H, W_, invalid_frac=0.02, seed=len(views))
        if lw is lw_in:
            base = np.where(base == 0, base, -0.3)                                # a wall 0.3 m in front
        cc = dict(c, lw=lw, dm=base)
        q = B.chain(cc)
        hit = np.unique((q["vi"] * W_ + q["ui"])[q["vis"]])
        dm, where = scatter_bad(base, hit, bad_values(ddt), rng)
        views.append((lw, dm))
        stats.append((cc, where))
    return c, views, stats


@pytest.mark.parametrize("ddt", [torch.float32, torch.float64], ids=["f32map", "f64map"])
@pytest.mark.parametrize("pinhole,res", [(True, (32, 32, 32)), (False, (32, 32, 32)), (True, (32, 32, 30)), (True, (24, 20, 160))],
                         ids=["pinhole", "skewed", "ragged", "bricks"])
def test_bad_depth_values(pinhole, res, ddt):
    """NaN, +-inf, wrong sign, +-0, -FLT_MAX, the smallest float32 subnormal and normal and -- float64 maps -- depths outside
    float32's range in both directions, scattered over three views (outside the grid, inside it, just in front of it), every
    sweep.  The oracle's rule is z = -depth, valid iff z > 0, in float64: NaN, positive and +-0 never update, huge finite depths
    update with min(tdist, sd) = tdist, -inf updates nothing (the reference's 0 * inf = NaN, see NEVER above), tiny depths update
    every voxel of their pixel with l2 < tdist + z -- voxels behind the camera among them."""
    c, views, stats = _bad_depth_views(pinhole, ddt, res)
    npdt = np.float32 if ddt == torch.float32 else np.float64
    To, Wo, masks, margin = check_all_sweeps(res, c["tsdf_res"], c["K"], c["Kinv"], c["scale"], c["center"], c["tdist"], 100.0, views, ddt)
    tiny_updates = tiny_behind = 0
    for (cc, where), (lw, dm), mask in zip(stats, views, masks):
        with np.errstate(all="ignore"):
            d = dm.astype(npdt)
            q = B.chain(cc, d)
        pix = q["vi"] * d.shape[1] + q["ui"]
        for name, val in bad_values(ddt):
            on_value = q["vis"] & np.isin(pix, where[name])
            assert int(on_value.sum()) >= 1, "no voxel projects to a pixel holding %s" % name
            stored = d.reshape(-1)[where[name]]
            assert np.array_equal(stored, np.full(stored.shape, npdt(val)), equal_nan=True)
            n_upd = int((mask & on_value).sum())
            if name in NEVER:
                assert n_upd == 0, name
            elif name in FAR:
                assert n_upd >= 1, name
                assert (q["sd"][mask & on_value] > cc["tdist"]).all()
            elif name in TINY:
                tiny_updates += n_upd
                tiny_behind += int((mask & on_value & (q["l2"] < 0)).sum())
        print("bad depths: view updates %d voxels; on tiny depths %d so far (%d behind the camera)" % (int(mask.sum()), tiny_updates, tiny_behind))
    assert tiny_updates >= 10 and tiny_behind >= 1                     # the camera inside the grid makes them visible


# --------------------------------------------------------------------------------------------------- d. path switch at 2048
@pytest.mark.parametrize("hw,want", [((16, 2048), "rows"), ((2048, 16), "rows"), ((16, 2049), "exact"), ((2049, 16), "exact")],
                         ids=["16x2048", "2048x16", "16x2049", "2049x16"])
def test_path_switch_at_2048_pixels(hw, want):
    """2^20 fixed-point pixel coordinates need (dim - 1) << 20 to fit int32: maps up to 2048 pixels take the fast path, larger
    ones the exact kernel.  A grid that is long along the map's long side, projections across (and beyond) its whole extent."""
    H, W_ = hw
    wide = W_ > H
    res = (64, 8, 16) if wide else (8, 64, 16)
    scale = scene.GRID_SIDE / 64
    center = scene.SPHERE_C + scale * (32.0 - np.array(res) / 2)                   # (index 32 maps to `center` on every axis: centre the slab-shaped grid)
    tdist = 4.0 * scale
    f_long, f_short = 0.5 * max(hw) / 0.39, 120.0                                  # the grid's long side spans 1.03 of the map's
    K = np.array([[f_long if wide else f_short, 0.0, W_ / 2 - 0.2713], [0.0, f_short if wide else f_long, H / 2 + 0.1371], [0.0, 0.0, 1.0]])
    Kinv = np.linalg.inv(K)
    lw = scene.view_extrinsic(0.0)
    lw[:, 3] += np.array([0.003, -0.002, 0.0])
    dm = scene.render_depth(K, lw, H, W_, invalid_frac=0.03, seed=2, dtype=np.float32)
    T = torch.empty(res, dtype=torch.float32)
    set_options({})
    assert kernels.integrate_path(T, torch.from_numpy(dm), res=res) == want
    assert kernels.integrate_path(T.double(), torch.from_numpy(dm), res=res) == "exact"
    c = dict(res=res, tsdf_res=64, K=K, Kinv=Kinv, lw=lw, scale=scale, center=center, tdist=tdist, dm=dm)
    q = B.chain(c)
    long_pix = q["ui"][q["vis"]] if wide else q["vi"][q["vis"]]
    print("path switch %dx%d: long-side pixels %d .. %d hit" % (H, W_, long_pix.min(), long_pix.max()))
    assert long_pix.min() <= 16 and long_pix.max() >= max(hw) - 17                 # projections span the whole extent (voxel pitch ~33 px)
    beyond = (q["u"] if wide else q["v"])[q["ok"]]
    assert (beyond < 0).any() and (beyond > max(hw) - 1).any()
    for ddt in (torch.float32, torch.float64):
        To, Wo, masks, margin = check_all_sweeps(res, 64, K, Kinv, scale, center, tdist, 100.0, [(lw, dm.astype(np.float64))] * 2, ddt)
        assert margin > 0 and 50 < int(masks[0].sum()) < Wo.size


# ------------------------------------------------------------------------------------- e. the association on bad depth values
def _canonical(R=64):
    H, W, fx, cx, cy = scene.CAMERAS["C1"]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(R)
    f = FusionDM(tdist, K, tsdf_res=R)
    T, Wt = f._new_volume_pair()
    for a in (0.0, 40.0, -40.0):
        lw = scene.view_extrinsic(a)
        dm = scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0)
        f.fuseDepths(torch.from_numpy(dm).cuda(), lw, T, Wt, scale=scale, center=center)
    return K, (H, W), scale, center, T, Wt


def _bad_frame(K, H, W, lws, scale, ddt, rng):
    """Live frames (the sphere displaced) with the bad values of c scattered over the sphere's pixels, one whole 16 x 16-pixel
    cell of NaN and one of -inf on the sphere."""
    npdt = np.float32 if ddt == torch.float32 else np.float64
    off = np.array([0.6, -0.4, 0.3]) * scale
    frames = []
    for i, lw in enumerate(lws):
        dm = scene.render_depth(K, lw, H, W, dtype=np.float64, invalid_frac=0.01, seed=5 + i, sphere_offset=off, wall_z=None)
        on_sphere = np.flatnonzero(dm.reshape(-1) != 0)
        dm, where = scatter_bad(dm, on_sphere, bad_values(ddt), rng, frac=0.15)
        for (r0, r1, c0, c1), val in ((NAN_CELL, np.nan), (INF_CELL, -np.inf)):
            assert r0 % 16 == 0 and c0 % 16 == 0 and r1 - r0 == 16 and c1 - c0 == 16
            dm[r0:r1, c0:c1] = val
        with np.errstate(over="ignore"):
            frames.append(np.ascontiguousarray(dm.astype(npdt)))
    return frames


def samples_on_bad_pixels(points_idx, K, lw_cam, dm, scale, center, half):
    """Per kind of bad depth, how many of the points project (visible, nearest pixel: the oracle's chain) onto a pixel holding it."""
    H, W = dm.shape
    cam = (scale * (np.asarray(points_idx, dtype=np.float64) - half) + center) @ lw_cam[:, :3].T + lw_cam[:, 3]
    u, v, ok = O.project_to_pixel(K, cam)
    vis = ok & (u >= 0) & (u < W - 1) & (v >= 0) & (v < H - 1)
    d = dm[np.rint(v[vis]).astype(np.int64), np.rint(u[vis]).astype(np.int64)].astype(np.float64)
    return {"nan": int(np.isnan(d).sum()), "-inf": int((d == -np.inf).sum()), "+inf": int((d == np.inf).sum()),
            "positive": int(((d > 0) & np.isfinite(d)).sum()), "zero": int((d == 0).sum()),
            "huge": int(((d <= -F32_MAX) & np.isfinite(d)).sum()), "tiny": int(((d < 0) & (d >= -F32_TINY)).sum()),
            "nan_cell": _in_block(u[vis], v[vis], NAN_CELL), "-inf_cell": _in_block(u[vis], v[vis], INF_CELL)}


NAN_CELL = (112, 128, 144, 160)        # rows, columns [r0, r1) x [c0, c1): cells (7, 9) and (7, 10) of the 16-pixel table
INF_CELL = (112, 128, 160, 176)


def _in_block(u, v, block):
    r0, r1, c0, c1 = block
    ui, vi = np.rint(u), np.rint(v)
    return int(((vi >= r0) & (vi < r1) & (ui >= c0) & (ui < c1)).sum())


@pytest.mark.parametrize("n_views", [1, 3, 4])
@pytest.mark.parametrize("ddt", [torch.float32, torch.float64], ids=["f32map", "f64map"])
def test_association_on_bad_depth_values(ddt, n_views):
    """dfh_gn_associate and the fused dfh_gn_build on frames that carry NaN, +-inf, wrong-sign, +-0, huge and tiny depths and whole
    16 x 16-pixel cells of NaN and of -inf (float32 frames: the cell table of view_cells_kernel; from four views on the fused build
    drops views per tile).  A non-finite correspondence is not a data row (oracle/gn_np.py:associate_depth): `valid` equals the
    oracle's, gated and ungated; the fused build equals associate-then-build bit for bit; nothing non-finite reaches corr of a
    valid sample, the system, the cost or -- after one dfh_gn_solve -- node_dq."""
    R, N, k = 64, 48, 4
    K, (H, W), scale, center, T, Wt = _canonical(R)
    Kinv = np.linalg.inv(K)
    lws = [scene.view_extrinsic(a) for a in (0.0, 40.0, -40.0, 20.0)][:n_views]
    rng = np.random.default_rng(23)
    frames = _bad_frame(K, H, W, lws, scale, ddt, rng)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    ident = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0, 0]), (N, 1))
    dq1 = G.apply_twists(ident, rng.normal(scale=[3e-3] * 3 + [0.2] * 3, size=(N, 6)))
    arg = (lambda ds: (ds, lws)) if n_views > 1 else (lambda ds: (ds[0], lws[0]))
    out = {}
    for mode in ("fused", "separate"):
        _lib.set_option("py_gn_no_fused_assoc", 1 if mode == "separate" else None)
        try:
            fs = FrameSolver(K, scale, center, R / 2, knn=k, pcg_iters=10, distributed=False)
            fs.set_graph(node_pos, ident, node_w)
            S = fs.set_canonical(T, Wt, band=2.0)
            sv = fs.solver
            ds = [torch.from_numpy(f).cuda() for f in frames]
            depth, lw_cam = arg(ds)
            pos = sv.spos.cpu().numpy()
            nbr = sv.snbr.cpu().numpy().astype(np.int64)
            snaps = []
            for dq, max_dist, huber in ((ident, 0.0, 0.0), (dq1, 2.0, 0.5), (dq1, 4.0, 0.0)):
                sv.node_dq.copy_(torch.from_numpy(dq).cuda())
                if mode == "separate":
                    # the association alone, against the oracle
                    sv.associate_depth(depth, fs.K, fs.Kinv, lw_cam, scale, center, R / 2, fs.lw, max_dist)
                    warped = O.warp(pos, dq[nbr], node_pos[nbr], node_w[nbr], m_lw=fs.lw)
                    with np.errstate(all="ignore"):
                        co, vo, view = G.associate_depth_views(warped, fs.K, fs.Kinv, lws, frames, scale, center, R / 2, max_dist=max_dist)
                    vg, cg = sv.valid.cpu().numpy().astype(bool), sv.corr.cpu().numpy()
                    assert np.isfinite(co[vo]).all()
                    assert np.array_equal(vg, vo), "valid differs from the oracle on %d samples (max_dist %g)" % (int((vg != vo).sum()), max_dist)
                    assert np.isfinite(cg[vg]).all()
                    # (1e-9 as on clean frames; relative for the huge correspondences of -FLT_MAX / -1e39 in the ungated case)
                    assert (np.abs(cg[vg] - co[vo]) <= 1e-9 * np.maximum(1.0, np.abs(co[vo]))).all()
                    print("association %d view(s) max_dist %g: %d of %d samples valid" % (n_views, max_dist, int(vo.sum()), S))
                    # the fixture's own conditions, from the oracle's side: in EVERY view each kind of bad depth sits under at least
                    # MIN_CLASS warped samples (so each view's gathers meet them, whichever view a sample ends up keeping), and
                    # both outcomes exist.  (With several views a sample that meets a bad pixel in one view is usually valid in
                    # another, so the count of invalid samples says little about what the views were fed.)
                    for lw_v, frame in zip(lws, frames):
                        hits = samples_on_bad_pixels(warped, fs.K, lw_v, frame, scale, center, R / 2)
                        print("   samples on bad pixels of one view: %s" % hits)
                        assert min(hits.values()) >= B.MIN_CLASS, hits
                    assert int(vo.sum()) > 500 and int((~vo).sum()) >= B.MIN_CLASS
                sv.build_associated(depth, fs.K, fs.Kinv, lw_cam, scale, center, R / 2, fs.lw, 0.7, max_dist, huber)
                torch.cuda.synchronize()
                snap = (sv.corr.clone(), sv.valid.clone(), sv.vals.clone(), sv.rhs.clone(), sv.cost_count.clone())
                assert bool(torch.isfinite(snap[0][snap[1].bool()]).all()), "non-finite corr of a valid sample"
                for name, t in zip(("vals", "rhs", "cost / count"), snap[2:]):
                    assert bool(torch.isfinite(t).all()), "non-finite %s (max_dist %g)" % (name, max_dist)
                snaps.append(snap)
            sv.node_dq.copy_(torch.from_numpy(ident).cuda())
            fs.gn_iteration(depth, lw_cam, max_dist=2.0, huber=0.5, n_iters=1)          # one dfh_gn_solve
            torch.cuda.synchronize()
            cost, cnt = sv.cost()
            assert np.isfinite(cost) and cnt > 500
            assert bool(torch.isfinite(sv.node_dq).all()) and bool(torch.isfinite(sv.vals).all()) and bool(torch.isfinite(sv.rhs).all())
            out[mode] = (snaps, (cost, cnt), sv.node_dq.clone())
        finally:
            _lib.set_option("py_gn_no_fused_assoc", None)
    for a, b in zip(out["fused"][0], out["separate"][0]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    assert out["fused"][1] == out["separate"][1] and torch.equal(out["fused"][2], out["separate"][2])
