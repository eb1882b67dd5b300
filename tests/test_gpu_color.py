"""GPU: K17, the colour volume fused through the warp field (dfh_integrate_color through kernels.integrate_color) and sampled at
points (dfh_sample_colors through kernels.sample_colors), against the numpy restatement (tests/color_np.py), against itself across
modes, views and slabs, and through FusionDM, Fusion and SlabFrame.

Bars.  Both sides gate on the same uploaded T / Wt, and what a voxel stores depends on the warped position only through
decisions (which pixel, inside the band or not): outside the voxels color_np.excluded() leaves out -- a decision within the last
ulps of its boundary, at most 0.5 % of the live voxels -- the set of changed voxels is the restatement's and C is torch.equal to it
(fp64 chain in a stated order, one rounding per component and view).  The colour volume starts from a random non-zero pattern,
so an untouched voxel is visible."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from dynamicfusion_body_amd import kernels, mesh, scene
from dynamicfusion_body_amd.pipeline import SlabFrame

import color_np as CN
import warped_np as WN

pytestmark = pytest.mark.gpu

INF = float("inf")


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))             # (a copy: the cached references are read-only arrays)
    return t.to("cuda", dtype=dtype or t.dtype)


@functools.lru_cache(maxsize=None)
def scene_of(name):
    if name == "skewed main":
        return WN.skewed_scene(scene_of("main"))
    return {"main": WN.main_scene, "ragged": WN.ragged_scene, "clustered": WN.clustered_scene}[name]()


@functools.lru_cache(maxsize=None)
def images(name):
    imgs = CN.color_images(scene_of(name))
    for i in imgs:
        i.setflags(write=False)
    return tuple(imgs)


@functools.lru_cache(maxsize=None)
def volumes(name, knn=4, dtype=np.float32):
    """The restatement's canonical volumes after the scene's two views, rounded to dtype: what both sides gate on."""
    T, Wt, _, _ = WN.restate(scene_of(name), knn)
    T, Wt = T.astype(dtype), Wt.astype(dtype)
    T.setflags(write=False)
    Wt.setflags(write=False)
    return T, Wt


@functools.lru_cache(maxsize=None)
def reference(name, knn, band, warp=True, wmax=100.0, calls=1, zero=False, dtype=np.float32):
    """The restatement's colour volume (from the pattern, or from zeros), computed once per case and never written to."""
    sc = scene_of(name)
    T, Wt = volumes(name, knn or 4, dtype)
    C = np.zeros(sc["shape"] + (4,), dtype=np.float32) if zero else CN.pattern(sc["shape"])
    ex = np.zeros(sc["shape"], dtype=bool)
    any_mask = np.zeros(sc["shape"], dtype=bool)
    for _ in range(calls):
        _, masks, mg = CN.restate(sc, knn, C, T, Wt, images(name), band, warp=warp, wmax=wmax)
        ex |= CN.excluded(mg)
        any_mask |= masks.any(axis=0)
    for a in (C, ex, any_mask):
        a.setflags(write=False)
    return C, any_mask, ex


def stored_ws(sc, knn, x_range=None):
    """A level-1 workspace whose index region a rebuilding integrate_depth_dqb call filled (on scratch volumes)."""
    a, b = (0, sc["shape"][0]) if x_range is None else x_range
    shape = (b - a,) + tuple(sc["shape"][1:])
    ws = kernels.dqb_workspace(sc["shape"], x_range, knn=knn, n_nodes=len(sc["node_pos"]), level=1)
    T = torch.full(shape, 1.0, dtype=torch.float32, device="cuda")
    kernels.integrate_depth_dqb(T, torch.zeros_like(T), [dev(d) for d in sc["depths"]], sc["K"], sc["Kinv"], sc["lws"], sc["scale"],
                                sc["center"], sc["tdist"], sc["node_pos"], sc["node_dq"], sc["node_w"], knn, sc["lw_dq"],
                                tsdf_res=sc["tsdf_res"], res=sc["shape"], x_range=x_range, workspace=ws, rebuild_candidates=True)
    return ws


def run(sc, C, T, Wt, imgs, band, knn=4, mode="search", ws=None, depths=None, lws=None, K=None, Kinv=None, node_dq=None, lw_dq=None,
        depth_dtype=None, x_range=None, **kw):
    """One kernels.integrate_color call; mode "none": no nodes, "search": the candidate lists (a fresh plain workspace unless one
    is given), "stored": the index region of `ws` (default: a fresh stored_ws)."""
    depths = sc["depths"] if depths is None else depths
    depths = [d if isinstance(d, torch.Tensor) else dev(d, depth_dtype) for d in depths]
    C = C if isinstance(C, torch.Tensor) else dev(C)
    T = T if isinstance(T, torch.Tensor) else dev(T)
    Wt = Wt if isinstance(Wt, torch.Tensor) else dev(Wt)
    nodes = {}
    if mode != "none":
        nodes = dict(node_pos=sc["node_pos"], node_dq=sc["node_dq"] if node_dq is None else node_dq, node_w=sc["node_w"], knn=knn,
                     lw_dq=sc["lw_dq"] if lw_dq is None else lw_dq)
        if mode == "stored":
            nodes.update(workspace=stored_ws(sc, knn, x_range) if ws is None else ws, stored_indices=True)
        elif ws is not None:
            nodes.update(workspace=ws)
    kernels.integrate_color(C, T, Wt, depths, list(imgs), sc["K"] if K is None else K, sc["Kinv"] if Kinv is None else Kinv,
                            sc["lws"] if lws is None else lws, sc["scale"], sc["center"], sc["tdist"], band, tsdf_res=sc["tsdf_res"],
                            res=sc["shape"] if x_range is not None else None, x_range=x_range, **nodes, **kw)
    return C


def compare(C, ref, start, live):
    """The device's colour volume against a restatement's (C, coloured mask, excluded)."""
    Co, upd, ex = ref
    assert ex.sum() <= WN.MAX_EXCLUDED * live.sum() and not (ex & ~live).any()
    keep = ~ex
    Cn = C.cpu().numpy()
    changed = np.any(Cn.view(np.uint32) != start.view(np.uint32), axis=-1)
    print("live %d, coloured %d of %d, excluded %d, mask mismatches outside the exclusions %d, differing packs %d"
          % (live.sum(), upd.sum(), upd.size, ex.sum(), (changed != upd)[keep].sum(),
             np.any(Cn.view(np.uint32) != Co.view(np.uint32), axis=-1)[keep].sum()))
    assert upd.any() and (~upd).any() and not (upd & ~live).any()
    assert np.array_equal(changed[keep], upd[keep])
    assert torch.equal(dev(Cn[keep]), dev(Co[keep]))


def live_of(T, Wt, band):
    with np.errstate(invalid="ignore"):
        return (Wt > 0) & (np.abs(T.astype(np.float64)) <= band)


# ---------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("mode", ["search", "stored"])
@pytest.mark.parametrize("name,knn,depth_dtype", [
    pytest.param("main", 1, None, id="main-1"), pytest.param("main", 3, None, id="main-3"), pytest.param("main", 4, None, id="main-4"),
    pytest.param("main", 8, None, id="main-8"), pytest.param("ragged", 4, None, id="ragged-4"),
    pytest.param("clustered", 4, None, id="clustered-4"), pytest.param("skewed main", 3, None, id="skewed main-3"),
    pytest.param("skewed main", 8, None, id="skewed main-8"), pytest.param("main", 3, torch.float64, id="main-3-float64 maps")])
def test_parity_with_the_restatement(name, knn, depth_dtype, mode):
    """Two views with different images through a non-rigid field.  ragged: no extent is a multiple of the brick; clustered: more
    than the 256 candidates a brick keeps, so the device scans every node; skewed main: the general projection chain (the volumes
    and the reference are the restatement's through the same K); float64 maps: the same values, the other load."""
    sc = scene_of(name)
    T, Wt = volumes(name, knn)
    start = CN.pattern(sc["shape"])
    C = run(sc, start, T, Wt, images(name), 1.5, knn=knn, mode=mode, depth_dtype=depth_dtype)
    compare(C, reference(name, knn, 1.5), start, live_of(T, Wt, 1.5))


# ---------------------------------------------------------------------------------------------- 2. the no-warp anchor
def skewed():
    return WN.skewed(scene_of("main")["K"])


@pytest.mark.parametrize("mode", ["search", "stored"])
@pytest.mark.parametrize("variant", ["plain", "skewed K", "float64 maps", "float64 volumes"])
def test_no_nodes_is_the_identity_field(variant, mode):
    sc = scene_of("main")
    N = len(sc["node_pos"])
    dtype = np.float64 if variant == "float64 volumes" else np.float32
    T, Wt = volumes("main", 4, dtype)
    kw = {}
    if variant == "skewed K":
        kw["K"], kw["Kinv"] = skewed()
        assert kw["Kinv"][2, 0] != 0 and kw["Kinv"][2, 1] != 0
    if variant == "float64 maps":
        kw["depth_dtype"] = torch.float64
    start = CN.pattern(sc["shape"])
    C0 = run(sc, start, T, Wt, images("main"), 2.0, mode="none", **kw)
    C1 = run(sc, start, T, Wt, images("main"), 2.0, knn=4, mode=mode, node_dq=np.tile(WN.IDENT, (N, 1)), lw_dq=WN.IDENT, **kw)
    assert not torch.equal(C0, dev(start)) and torch.equal(C0, C1)
    # ... and the no-warp call is the restatement's, with nothing left out but the pixel ties and band edges
    if variant in ("plain", "float64 volumes"):
        compare(C0, reference("main", None, 2.0, warp=False, dtype=dtype), start, live_of(T, Wt, 2.0))


# ---------------------------------------------------------------------------------------------- 3. views and slabs
@pytest.mark.parametrize("mode", ["none", "search", "stored"])
def test_views_in_one_call_are_one_call_per_view(mode):
    sc = scene_of("main")
    T, Wt = volumes("main")
    imgs = images("main")
    ws = stored_ws(sc, 4) if mode == "stored" else None
    C = run(sc, CN.pattern(sc["shape"]), T, Wt, imgs, 1.5, mode=mode, ws=ws, wmax=5.0)
    C2 = dev(CN.pattern(sc["shape"]))
    for v in range(2):
        run(sc, C2, T, Wt, imgs[v:v + 1], 1.5, mode=mode, ws=ws, wmax=5.0, depths=sc["depths"][v:v + 1], lws=sc["lws"][v:v + 1])
    assert torch.equal(C, C2) and bool((C[..., 3] == 5.0).any())


def test_nineteen_views_go_sixteen_at_a_time():
    sc = scene_of("ragged")
    T, Wt = volumes("ragged")
    rng = np.random.default_rng(19)
    H, W = sc["depths"][0].shape
    depths = [dev(sc["depths"][i % 2]) for i in range(19)]
    lws = [sc["lws"][i % 2] for i in range(19)]
    imgs = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(19)]           # (H, W, 3): padded by the wrapper
    C = run(sc, CN.pattern(sc["shape"]), T, Wt, imgs, 2.0, mode="search", depths=depths, lws=lws, wmax=12.0)
    C2 = dev(CN.pattern(sc["shape"]))
    for v in range(19):
        run(sc, C2, T, Wt, imgs[v:v + 1], 2.0, mode="search", depths=depths[v:v + 1], lws=lws[v:v + 1], wmax=12.0)
    assert torch.equal(C, C2) and bool((C[..., 3] == 12.0).any())


@pytest.mark.parametrize("mode", ["none", "search", "stored"])
def test_slabs_equal_the_whole_grid(mode):
    sc = scene_of("main")
    T, Wt = volumes("main")
    start = CN.pattern(sc["shape"])
    whole = run(sc, start, T, Wt, images("main"), 1.5, mode=mode)
    halves = dev(start)
    for a, b in ((0, 16), (16, 32)):
        Cs = run(sc, start[a:b], T[a:b], Wt[a:b], images("main"), 1.5, mode=mode, x_range=(a, b))
        halves[a:b] = Cs
    assert torch.equal(halves, whole)
    # a slab that cuts bricks at both ends
    Cs = run(sc, start[3:13], T[3:13], Wt[3:13], images("main"), 1.5, mode=mode, x_range=(3, 13))
    assert torch.equal(Cs, whole[3:13]) and not torch.equal(Cs, dev(start[3:13]))


def test_an_empty_slab_and_no_views_touch_nothing():
    sc = scene_of("main")
    Te = torch.empty((0, 32, 32), dtype=torch.float32, device="cuda")
    Ce = torch.empty((0, 32, 32, 4), dtype=torch.float32, device="cuda")
    assert run(sc, Ce, Te, Te.clone(), images("main"), 1.5, mode="none", x_range=(9, 9)) is Ce
    T, Wt = volumes("main")
    start = CN.pattern(sc["shape"])
    C = run(sc, start, T, Wt, [], 1.5, mode="search", depths=[], lws=[])
    assert torch.equal(C, dev(start))


# ---------------------------------------------------------------------------------------------- 4. gates
def test_dead_voxels_keep_their_pattern():
    """w == 0, |T| > band and T = NaN planted on voxels that would otherwise be coloured."""
    sc = scene_of("main")
    T0, W0 = volumes("main")
    _, upd, _ = reference("main", 4, 1.5)
    idx = np.argwhere(upd)
    assert len(idx) > 300
    T, Wt = T0.copy(), W0.copy()
    dead = np.zeros(sc["shape"], dtype=bool)
    for j, i in enumerate(idx[::2]):
        i = tuple(i)
        dead[i] = True
        if j % 3 == 0:
            Wt[i] = 0.0
        elif j % 3 == 1:
            T[i] = np.float32(1.5) + np.spacing(np.float32(1.5)) if j % 2 else -np.float32(1.5) - np.spacing(np.float32(1.5))
        else:
            T[i] = np.nan
    start = CN.pattern(sc["shape"])
    Cr = start.copy()
    _, masks, mg = CN.restate(sc, 4, Cr, T, Wt, images("main"), 1.5)
    assert not (masks.any(axis=0) & dead).any()
    for mode in ("none", "search", "stored"):
        C = run(sc, start, T, Wt, images("main"), 1.5, mode=mode)
        assert torch.equal(C[dev(dead)], dev(start[dead]))
        if mode == "search":
            compare(C, (Cr, masks.any(axis=0), CN.excluded(mg)), start, live_of(T, Wt, 1.5))


@pytest.mark.parametrize("mode", ["none", "search", "stored"])
def test_band_below_every_voxel_and_infinite_band(mode):
    sc = scene_of("main")
    T, Wt = volumes("main")
    start = CN.pattern(sc["shape"])
    low = float(np.abs(T[Wt > 0]).min()) / 2
    assert low > 0
    assert torch.equal(run(sc, start, T, Wt, images("main"), low, mode=mode, band_sd=1.5 * sc["scale"]), dev(start))
    # band_vox = +inf: every w > 0 voxel that a view sees inside band_sd
    C = run(sc, start, T, Wt, images("main"), INF, mode=mode, band_sd=1.5 * sc["scale"])
    Cr = start.copy()
    _, masks, mg = CN.restate(sc, 4, Cr, T, Wt, images("main"), INF, warp=mode != "none", band_sd=1.5 * sc["scale"])
    live = Wt > 0
    assert masks.any(axis=0).sum() > reference("main", 4, 1.5)[1].sum()
    compare(C, (Cr, masks.any(axis=0), CN.excluded(mg)), start, live)
    # ... and with band_sd = +inf too, every w > 0 voxel some view measures at all
    C = run(sc, start, T, Wt, images("main"), INF, mode=mode, band_sd=INF)
    Cr = start.copy()
    _, masks, mg = CN.restate(sc, 4, Cr, T, Wt, images("main"), INF, warp=mode != "none", band_sd=INF)
    compare(C, (Cr, masks.any(axis=0), CN.excluded(mg)), start, live)


@pytest.mark.parametrize("depth_dtype", [torch.float32, torch.float64])
def test_bad_depth_values_colour_nothing(depth_dtype):
    sc = scene_of("main")
    T, Wt = volumes("main")
    H, W = sc["depths"][0].shape
    start = CN.pattern(sc["shape"])
    bad = [np.full((H, W), v, dtype=np.float32) for v in (0.0, np.nan, -np.inf, np.inf)]
    imgs = [images("main")[0]] * 4
    lws = [sc["lws"][0], sc["lws"][1]] * 2
    for mode in ("none", "search"):
        C = run(sc, start, T, Wt, imgs, INF, mode=mode, depths=bad, lws=lws, band_sd=INF, depth_dtype=depth_dtype)
        assert torch.equal(C, dev(start))
    # stripes of them under the sphere: those pixels colour nothing, the others do what the restatement does
    depths = [d.copy() for d in sc["depths"]]
    for d in depths:
        d[100:140:4, 120:200] = 0.0
        d[101:140:4, 120:200] = -np.inf
        d[102:140:4, 120:200] = np.nan
        d[103:140:4, 120:200] = np.inf
    Cr = start.copy()
    _, masks, mg = CN.restate(sc, 4, Cr, T, Wt, images("main"), 1.5, depths=depths)
    _, plain, _ = CN.restate(sc, 4, start.copy(), T, Wt, images("main"), 1.5)
    assert (plain[0] & ~masks[0]).sum() > 20 and (plain[1] & ~masks[1]).sum() > 20          # the bad pixels lie under band voxels
    C = run(sc, start, T, Wt, images("main"), 1.5, mode="search", depths=depths, depth_dtype=depth_dtype)
    assert bool(torch.isfinite(C).all())
    compare(C, (Cr, masks.any(axis=0), CN.excluded(mg)), start, live_of(T, Wt, 1.5))


# ---------------------------------------------------------------------------------------------- 5. the weight cap
def test_weight_cap():
    sc = scene_of("main")
    T, Wt = volumes("main")
    zero = np.zeros(sc["shape"] + (4,), dtype=np.float32)
    C = dev(zero)
    ws = stored_ws(sc, 4)
    for _ in range(5):
        run(sc, C, T, Wt, images("main"), 1.5, mode="stored", ws=ws, wmax=3.0)
    ref = reference("main", 4, 1.5, wmax=3.0, calls=5, zero=True)
    compare(C, ref, zero, live_of(T, Wt, 1.5))
    wc = C[..., 3]
    assert float(wc.max()) == 3.0 and bool(((wc == 0) | (wc == 3.0)).all())
    # the colour of a voxel both views see keeps moving under the cap: it is not the value of the first three updates
    three = reference("main", 4, 1.5, wmax=3.0, calls=2, zero=True)[0]
    assert np.any(three[..., :3] != ref[0][..., :3])


# ---------------------------------------------------------------------------------------------- 6. determinism, read-only inputs
@pytest.mark.parametrize("mode", ["search", "stored"])
def test_same_bits_every_run_and_inputs_untouched(mode):
    sc = scene_of("clustered")
    N = len(sc["node_pos"])
    T, Wt = volumes("clustered")
    Td, Wd = dev(T), dev(Wt)
    ws = kernels.dqb_workspace(sc["shape"], knn=4, n_nodes=N, level=2)
    ws.fill_(0x5a5a5a5a)                                              # (the weight region is nobody's here: it must stay as it is)
    kernels.integrate_depth_dqb(Td.clone(), Wd.clone(), [dev(d) for d in sc["depths"]], sc["K"], sc["Kinv"], sc["lws"], sc["scale"],
                                sc["center"], sc["tdist"], sc["node_pos"], sc["node_dq"], sc["node_w"], 4, sc["lw_dq"],
                                tsdf_res=sc["tsdf_res"], workspace=ws, rebuild_candidates=True)
    before = ws.clone()
    kw = dict(workspace=ws, stored_indices=True) if mode == "stored" else dict(workspace=ws)
    outs = []
    for _ in range(2):
        C = dev(CN.pattern(sc["shape"]))
        kernels.integrate_color(C, Td, Wd, [dev(d) for d in sc["depths"]], list(images("clustered")), sc["K"], sc["Kinv"], sc["lws"],
                                sc["scale"], sc["center"], sc["tdist"], 1.5, sc["node_pos"], sc["node_dq"], sc["node_w"], 4,
                                sc["lw_dq"], tsdf_res=sc["tsdf_res"], **kw)
        outs.append(C)
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], dev(CN.pattern(sc["shape"])))
    assert torch.equal(ws, before) and torch.equal(Td, dev(T)) and torch.equal(Wd, dev(Wt))


# ---------------------------------------------------------------------------------------------- 7. sample_colors
@functools.lru_cache(maxsize=None)
def sample_case():
    rng = np.random.default_rng(23)
    R = (32, 24, 20)
    C = rng.uniform(0.0, 255.0, size=R + (4,)).astype(np.float32)
    C[..., 3] = np.where(rng.random(R) < 0.5, 0.0, rng.integers(1, 9, size=R)).astype(np.float32)
    C[:8, :8, :8, 3] = 0.0                                            # a corner of the grid nobody coloured
    top = np.array(R, dtype=np.float64) - 1
    pts = [rng.uniform(-1.0, 1.0, size=(2200, 3)) * 0.55 * (top + 2) + top / 2,           # inside, with some outside
           rng.integers(0, 20, size=(500, 3)).astype(np.float64),                        # lattice points
           rng.uniform(0.0, 7.0, size=(250, 3)),                                         # all eight corners have wc = 0
           rng.uniform(8.5, 20.5, size=(650, 3)) * np.array([1.0, 1.0, 0.9])]            # round the slab [10, 20) below
    for axis in range(3):                                             # on the last plane of each axis, and just beyond it
        p = rng.uniform(0.0, 1.0, size=(100, 3)) * top
        p[:, axis] = top[axis]
        p[50:75, axis] = np.nextafter(top[axis], np.inf)
        p[75:, axis] = np.nextafter(top[axis], 0.0)
        pts.append(p)
    odd = rng.uniform(1.0, 15.0, size=(196, 3))
    odd[:60, 0] = np.nan
    odd[60:100, 1] = np.inf
    odd[100:140, 2] = -np.inf
    odd[140:170, 0] = -1e-300
    odd[170:, 1] = -0.0                                               # (inside: -0.0 >= 0)
    pts.append(odd)
    pts = np.concatenate(pts)
    assert pts.shape == (4096, 3)
    return C, pts, R


def test_sample_colors_is_the_restatement():
    C, pts, R = sample_case()
    rgb, valid = kernels.sample_colors(dev(C), dev(pts))
    rgb_o, valid_o = CN.sample_colors_np(C, pts)
    assert 0.3 < valid_o.mean() < 0.9 and not valid_o[2700:2950].any() and valid_o[-26:].any()
    assert rgb.dtype == torch.float32 and valid.dtype == torch.bool
    assert torch.equal(valid, dev(valid_o)) and torch.equal(rgb, dev(rgb_o))
    # a slab: points between planes 9 and 10 see only their upper x plane, between 19 and 20 only their lower one
    rgb_s, valid_s = kernels.sample_colors(dev(C[10:20]), dev(pts), x_range=(10, 20), res=R)
    rgb_so, valid_so = CN.sample_colors_np(C[10:20], pts, res=R, x_range=(10, 20))
    edge = ((pts[:, 0] > 9) & (pts[:, 0] < 10)) | ((pts[:, 0] > 19) & (pts[:, 0] < 20))
    assert (valid_so & edge).sum() > 50 and np.any(rgb_so[valid_so & edge] != rgb_o[valid_so & edge])
    assert torch.equal(valid_s, dev(valid_so)) and torch.equal(rgb_s, dev(rgb_so))
    inner = (pts[:, 0] >= 10) & (pts[:, 0] <= 19)
    assert np.array_equal(rgb_so[inner], rgb_o[inner])
    # nothing to do
    rgb_e, valid_e = kernels.sample_colors(dev(C), torch.empty((0, 3), dtype=torch.float64, device="cuda"))
    assert rgb_e.shape == (0, 3) and valid_e.shape == (0,)


# ---------------------------------------------------------------------------------------------- 8. recovery
def test_recovery_of_a_painted_sphere():
    """FusionDM.compute_live_tsdf(colors=...) on the sphere painted with a smooth colour field (color_np.recovery_scene), marching
    cubes, sample_colors: the device's vertex colours are the restatement's (from the device's volumes and vertices), and their
    error against the colour field is the one recorded in tests/golden/color_recovery.json (rms 4.03 of 255 at 32^3, 42 % of the
    level-0 vertices coloured -- see tests/test_color_np.py for the rest)."""
    from dynamicfusion_body_amd import FusionDM
    s = CN.recovery_scene()
    f = FusionDM(s["tdist"], s["K"], tsdf_res=s["res"], volume_dtype=np.float64)
    T, Wt = f.compute_live_tsdf(s["depths"], s["lws"], UseAutoAlignment=True, as_numpy=False, colors=s["colors"],
                                color_band=CN.RECOVERY_BAND)
    assert f._C is not None and tuple(f._C.shape) == (32, 32, 32, 4)
    verts, faces, normals, _ = mesh.marching_cubes(T, 0.0, 1)
    rgb, valid = kernels.sample_colors(f._C, verts.double())
    Co, rgb_o, valid_o = CN.recovery_colors(s, T.cpu().numpy(), Wt.cpu().numpy(), verts.cpu().numpy())
    assert torch.equal(f._C, dev(Co))
    assert torch.equal(valid, dev(valid_o)) and torch.equal(rgb[valid], dev(rgb_o)[valid])
    got = CN.recovery_metrics(s, verts.cpu().numpy(), rgb.cpu().numpy(), valid.cpu().numpy())
    rec = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_recovery.json")))
    print(got, rec)
    assert got["n_vertices"] == rec["n_vertices"]
    assert abs(got["rms"] - rec["rms"]) <= 1e-6 and abs(got["valid_share"] - rec["valid_share"]) <= 1e-6
    # without colours the object has no colour volume; with useICP colours are refused
    f.compute_live_tsdf(s["depths"], s["lws"], UseAutoAlignment=True, as_numpy=False)
    assert f._C is None
    with pytest.raises(ValueError, match="useICP"):
        f.compute_live_tsdf(s["depths"], s["lws"], useICP=True, colors=s["colors"])


def test_fusion_dm_writes_a_coloured_mesh(tmp_path):
    from dynamicfusion_body_amd import FusionDM
    s = CN.recovery_scene()
    f = FusionDM(s["tdist"], s["K"], tsdf_res=s["res"])
    f.compute_live_tsdf(s["depths"], s["lws"], UseAutoAlignment=True, as_numpy=False, colors=s["colors"])
    f.write_canonical_mesh(str(tmp_path), "c.obj")
    verts, faces, normals, _ = mesh.marching_cubes(f._T, 0.0, 1)
    rgb, valid = kernels.sample_colors(f._C, verts.double())
    got = mesh.read_obj_colors(str(tmp_path / "c.obj"))
    want = mesh.obj_colors(rgb.cpu().numpy(), valid.cpu().numpy(), len(verts))
    assert got.shape == (len(verts), 3) and np.abs(got - want).max() <= 5e-7
    assert bool(valid.any()) and bool((~valid).any()) and np.all(got[~valid.cpu().numpy()] == 0.5)
    f._C = None
    f.write_canonical_mesh(str(tmp_path), "plain.obj")
    assert mesh.read_obj_colors(str(tmp_path / "plain.obj")) is None
    for a, b in zip(mesh.read_obj(str(tmp_path / "plain.obj")), mesh.read_obj(str(tmp_path / "c.obj"))):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------- 9. the frame loop
R, N = 32, 48
ANGLES = (0.0, 40.0)


@functools.lru_cache(maxsize=None)
def frames(n=3):
    H, W, fx, cx, cy = scene.CAMERAS["C1"]
    K = scene.intrinsics(fx, cx, cy)
    scale = scene.grid_params(R)[0]
    lws = [scene.view_extrinsic(a) for a in ANGLES]
    rng = np.random.default_rng(17)
    depth, color = [], []
    for f in range(n + 1):                          # frame 0 builds the canonical volume
        off = np.array([0.4, -0.25, 0.15]) * f * scale                # a translating sphere
        depth.append([torch.from_numpy(scene.render_depth(K, lw, H, W, dtype=np.float32, invalid_frac=0.0, sphere_offset=off)).cuda()
                      for lw in lws])
        color.append([rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in lws])
    return K, lws, depth, color


def new_loop(K, lws, first, color_band=None):
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=2.0, distributed=False,
                   color_band=color_band)
    for d, lw in zip(first, lws):
        sf.integrate(d, lw)
    assert sf.refresh_samples() > 100
    return sf


@pytest.mark.parametrize("update", ["volume", "depth"])
def test_frame_loop_with_colours(update):
    K, lws, depth, color = frames()
    a, b = new_loop(K, lws, depth[0]), new_loop(K, lws, depth[0], color_band=1.5)
    assert a.C is None and tuple(b.C.shape) == (R, R, R, 4) and not bool(b.C.any())
    for ds, cs in zip(depth[1:], color[1:]):
        wc0 = b.C[..., 3].clone()
        na = a.step(ds, lws, gn_iters=4, update=update)
        nb = b.step(ds, lws, gn_iters=4, update=update, colors=cs)
        assert na == nb
        # colour reads everything else and writes only C
        sa, sb = a.fs.solver, b.fs.solver
        assert torch.equal(a.T, b.T) and torch.equal(a.Wt, b.Wt) and torch.equal(sa.node_dq, sb.node_dq)
        assert torch.equal(sa.spos, sb.spos) and torch.equal(sa.snrm, sb.snrm)
        grown = b.C[..., 3] != wc0
        band = (b.Wt > 0) & (b.T.abs() <= 1.5)
        assert bool(grown.any()) and not bool((grown & ~band).any())
        assert bool((b.C[..., 3] >= wc0).all())
    assert float(b.C[..., 3].max()) > 2.0
    verts, faces, normals, rgb, valid = b.colored_mesh()
    assert verts.shape[0] > 100 and faces.shape[0] > 100 and rgb.shape == verts.shape and bool(valid.any())
    assert float(rgb[valid].min()) >= 0.0 and float(rgb[valid].max()) <= 255.0
    with pytest.raises(ValueError, match="color_band"):
        a.step(depth[1], lws, gn_iters=1, update=update, colors=color[1])
    with pytest.raises(ValueError, match="color_band"):
        a.colored_mesh()
    with pytest.raises(ValueError, match="one colour image per depth map"):
        b.step(depth[1], lws, gn_iters=1, update=update, colors=color[1][:1])


def test_one_frame_is_one_colour_call():
    """The frame's colour call is kernels.integrate_color with the field the update used (before it decays), the update's
    workspace and its stored indices."""
    K, lws, depth, color = frames()
    b = new_loop(K, lws, depth[0], color_band=1.5)
    b.step(depth[1], lws, gn_iters=4, update="depth", colors=color[1])
    C0 = b.C.clone()
    b.step(depth[2], lws, gn_iters=4, update="depth", colors=color[2], relax=1.0)
    sv = b.fs.solver
    kernels.integrate_color(C0, b.T, b.Wt, depth[2], color[2], b.K, b.Kinv, lws, b.scale, b.center, b.tdist_world, 1.5, sv.node_pos,
                            sv.node_dq, sv.node_w, 4, b.ident_lw, tsdf_res=R)
    assert torch.equal(b.C, C0) and not torch.equal(sv.node_dq, torch.tensor(b.ident_lw, device="cuda").expand(N, 8))


def test_fusion_update_tsdf_depths_with_colours(tmp_path):
    from dynamicfusion_body_amd import Fusion
    sc = scene_of("main")
    T0, W0 = WN.start_volumes(sc, np.float32)
    f = Fusion(T0.copy(), sc["tdist"], knn=4, volume_dtype=np.float32)
    f._tsdfw = W0
    f._K, f._Kinv = sc["K"], sc["Kinv"]
    f._nodes = [(0, sc["node_pos"][i], sc["node_dq"][i], float(sc["node_w"][i])) for i in range(len(sc["node_pos"]))]
    f._lw = sc["lw_dq"]
    f.updateTSDF_depths(sc["depths"], sc["lws"], wmax=7.0, scale=sc["scale"], center=sc["center"], colors=images("main"))
    assert f._C is not None
    C = run(sc, np.zeros(sc["shape"] + (4,), dtype=np.float32), f._T, f._Wt, images("main"), 1.5, mode="search")
    assert torch.equal(f._C, C) and bool((C[..., 3] > 0).any())
    f.write_canonical_mesh(str(tmp_path), "c.obj")
    verts, faces, normals, _ = mesh.marching_cubes(f._T, None, 1)
    rgb, valid = kernels.sample_colors(f._C, verts.double())
    got = mesh.read_obj_colors(str(tmp_path / "c.obj"))
    want = mesh.obj_colors(rgb.cpu().numpy(), valid.cpu().numpy(), len(verts))
    assert got.shape == (len(verts), 3) and np.abs(got - want).max() <= 5e-7 and bool(valid.any())
    assert np.array_equal(mesh.read_obj(str(tmp_path / "c.obj"))[0].shape, (len(verts), 3))


def test_fusion_initialize_canonical_space_with_colours():
    """InitializeCanonicalSpace(depths=..., colors=...) fuses the colours with no warp, after its sweep; without colours (and from a
    given tsdf) the object has no colour volume."""
    from dynamicfusion_body_amd import Fusion
    s = CN.recovery_scene()
    fu = Fusion(np.zeros((4, 4, 4)), s["tdist"], knn=4, write_warpfield=False)
    fu.InitializeCanonicalSpace(depths=s["depths"], lws=s["lws"], K=s["K"], tsdf_size=32, scale=s["scale"], center=s["center"],
                                colors=s["colors"], color_band=2.0)
    C = kernels.color_volume((32, 32, 32))
    kernels.integrate_color(C, fu._T, fu._Wt, [dev(d) for d in s["depths"]], s["colors"], s["K"], s["Kinv"], s["lws"], s["scale"],
                            s["center"], s["tdist"], 2.0)
    assert torch.equal(fu._C, C) and int((C[..., 3] > 0).sum()) > 100
    Co = np.zeros((32, 32, 32, 4), dtype=np.float32)
    CN.integrate_color_np(Co, fu._T.cpu().numpy(), fu._Wt.cpu().numpy(), s["depths"], s["colors"], s["lws"], s["K"], s["Kinv"],
                          s["scale"], s["center"], s["tdist"], 2.0, 2.0 * s["scale"])
    assert torch.equal(C, dev(Co))
    fu.InitializeCanonicalSpace(depths=s["depths"], lws=s["lws"], K=s["K"], tsdf_size=32, scale=s["scale"], center=s["center"])
    assert fu._C is None
    with pytest.raises(ValueError, match="one colour image per depth map"):
        fu.InitializeCanonicalSpace(depths=s["depths"], lws=s["lws"], K=s["K"], tsdf_size=32, colors=s["colors"][:1])
