"""GPU: the RGB-D ingest kernels (kernels.rgbd_ingest, dfh_rgbd_ingest) against their numpy restatement (tests/ingest_np.py), bit
for bit on all three outputs and on the z-buffer, at every pixel -- every operation of the stage is an IEEE basic operation in a
stated order, so there is no tolerance -- and the hooks (RGBDIngest, SlabFrame(ingest=), FusionDM.ingest, Fusion.ingest) against the stage called
by hand."""
import functools

import numpy as np
import pytest
import torch

import depth_prep_cases as DC
import ingest_cases as C
import ingest_np as N
from dynamicfusion_body_amd import FusionDM, kernels, scene
from dynamicfusion_body_amd.ingest import DEFAULT_OCCL_TOL, RGBDCalibration, RGBDIngest
from dynamicfusion_body_amd.pipeline import SlabFrame

pytestmark = pytest.mark.gpu

SAMPLE = {0: "nearest", 1: "bilinear"}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(raw, img, views, out_k, out=None, workspace=None, **kw):
    """kernels.rgbd_ingest on numpy inputs -> numpy (depth, color, color_depth, zbuf uint32); the inputs are only read."""
    kw = dict(kw)
    kw["sample"] = SAMPLE[kw.get("sample", 1)]
    d = [torch.from_numpy(np.ascontiguousarray(r).view(np.int16)).cuda() for r in raw]
    c = None if img is None else [torch.from_numpy(np.ascontiguousarray(m)).cuda() for m in img]
    got = kernels.rgbd_ingest(d, c, views, out_k, out=out, workspace=workspace, **kw)
    torch.cuda.synchronize()
    for r, t in zip(raw, d):
        assert np.array_equal(t.cpu().numpy().view(np.uint16), r)
    if img is not None:
        for m, t in zip(img, c):
            assert np.array_equal(t.cpu().numpy(), m)
    depth, color, cdepth, zbuf = (None if t is None else t.cpu().numpy() for t in got)
    return depth, color, cdepth, None if zbuf is None else zbuf.view(np.uint32)


def same(got, want):
    """All four results, bit for bit (float maps as their bit patterns: -0.0 is not 0.0)."""
    for name, g, w in zip(("depth", "color", "color_depth", "zbuf"), got, want):
        if w is None:
            assert g is None, name
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float32:
            g, w = bits(g), bits(w)
        diff = g != w
        assert not diff.any(), (name, int(diff.sum()), np.argwhere(diff)[:5])


# ---- sizes: tile edges, view counts, colour smaller / equal / 2.5 x, 3 and 4 channels, both samplers, no colour ------------------
def tile_shape(dh, dw):
    th, tw = kernels.rgbd_ingest_tile()
    return th + dh, tw + dw


# name -> (depth size or tile offsets, views, colour scale or None, C, sample, distortion)
SIZE_CASES = {
    "2x2 1 view, colour equal": ((2, 2), 1, 1.0, 3, 1, False),
    "2x2 3 views, no colour": ((2, 2), 3, None, 3, 1, False),
    "tile-1 3 views, colour 2.5x, C4 bilinear": ("-1-1", 3, 2.5, 4, 1, False),
    "tile 1 view, colour equal, C3 nearest": ("+0+0", 1, 1.0, 3, 0, False),
    "tile 16 views, colour smaller, C4 nearest": ("+0+0", 16, 0.5, 4, 0, False),
    "tile+1 3 views, colour 2.5x, C3 bilinear": ("+1+1", 3, 2.5, 3, 1, False),
    "tile+1 -1 16 views, colour equal, C3 bilinear": ("+1-1", 16, 1.0, 3, 1, False),
    "tile-1 +1 1 view, colour smaller, C3 bilinear": ("-1+1", 1, 0.5, 3, 1, False),
    "tile+1 16 views, no colour": ("+1+1", 16, None, 3, 1, False),
    "2 tiles + 1, 3 views, distortion on both cameras": ("x2", 3, 2.5, 4, 1, True),
    "tile 1 view, distortion, no colour": ("+0+0", 1, None, 3, 1, True),
}


def size_case(name):
    shape, V, cs, ch, sample, dist = SIZE_CASES[name]
    if shape == "x2":
        th, tw = kernels.rgbd_ingest_tile()
        shape = (2 * th + 1, 2 * tw + 1)
    elif isinstance(shape, str):
        shape = tile_shape(int(shape[:2]), int(shape[2:]))
    color_size = None if cs is None else (max(2, int(round(shape[0] * cs))), max(2, int(round(shape[1] * cs))))
    raw, img, views, out_k = C.random_frame(len(name), V, shape, color_size, C=ch, distortion=dist)
    return (raw, img, views, out_k), dict(sample=sample, occl_tol=DEFAULT_OCCL_TOL, max_splat=8)


@functools.lru_cache(maxsize=None)
def size_reference(name):
    """(args, kw, the restatement's results): computed once, read-only."""
    args, kw = size_case(name)
    want = N.ingest(*args, **kw)
    for a in want:
        if a is not None:
            a.setflags(write=False)
    return args, kw, want


@pytest.mark.parametrize("name", sorted(SIZE_CASES))
def test_sizes(name):
    args, kw, want = size_reference(name)
    if want[1] is not None and args[0].shape[1] > 2:
        assert (want[1][..., 3] == 255).any() and (want[3] != N.EMPTY).any(), "the case registers no colour at all"
    same(run(*args, **kw), want)


# ---- decisions on representable boundaries --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.BOUNDARY_CASES))
def test_boundaries(name):
    case = C.BOUNDARY_CASES[name]()
    got = run(*case["args"], **case["kw"])
    case["check"](got)                                              # what tests/test_ingest.py asserts of the restatement
    same(got, N.ingest(*case["args"], **case["kw"]))


# ---- geometry edges ---------------------------------------------------------------------------------------------------------------
def geometry_case(name):
    shape, color = (9, 70), (22, 175)
    kw = dict(sample=1, occl_tol=DEFAULT_OCCL_TOL, max_splat=8)
    if name == "behind the colour camera":          # Pc_2 = z - 1.9 with z in 1.2 .. 2.7: pixels on both sides of 0
        T = np.hstack([np.eye(3), np.array([[0.05], [0.0], [-1.9]])])
        args = C.random_frame(41, 2, shape, color, T=T)
    elif name == "rectangle wider than max_splat":  # a depth pixel covers 2.5 colour pixels, cut to 2 and to 1
        args = C.random_frame(42, 2, shape, color)
        kw["max_splat"] = 2
    elif name == "max_splat 1":
        args = C.random_frame(43, 1, shape, color)
        kw["max_splat"] = 1
    elif name == "max_splat 16, colour 6x":
        args = C.random_frame(44, 1, (5, 9), (30, 54))
        kw["max_splat"] = 16
    elif name == "rectangles across the border":    # shifted half an image to the left and up
        T = np.hstack([np.eye(3), np.array([[-0.9], [-0.12], [0.0]])])
        args = C.random_frame(45, 2, shape, color, T=T)
    elif name == "an all-invalid map among others":
        args = list(C.random_frame(46, 3, shape, color))
        args[0] = args[0].copy()
        args[0][1] = 0
        args = tuple(args)
    elif name == "all maps invalid":
        args = list(C.random_frame(47, 2, shape, color))
        args[0] = np.zeros_like(args[0])
        args = tuple(args)
    elif name == "no occlusion test":
        args = C.random_frame(48, 2, shape, color)
        kw["occl_tol"] = float("inf")
    elif name == "z range":
        args = C.random_frame(49, 2, shape, color)
        kw.update(z_min=1.4, z_max=2.2)
    else:
        raise KeyError(name)
    return args, kw


GEOMETRY = ["behind the colour camera", "rectangle wider than max_splat", "max_splat 1", "max_splat 16, colour 6x",
            "rectangles across the border", "an all-invalid map among others", "all maps invalid", "no occlusion test", "z range"]


@pytest.mark.parametrize("name", GEOMETRY)
def test_geometry_edges(name):
    args, kw = geometry_case(name)
    want = N.ingest(*args, **kw)
    has = want[1][..., 3] == 255
    if name == "behind the colour camera":
        raw, views = args[0], args[2]
        z = raw.astype(np.float64) * 1e-3
        assert ((raw != 0) & (z < 1.9)).sum() > 50 and ((z > 1.9)).sum() > 50 and has.any()
    elif name == "all maps invalid":
        assert not has.any() and (want[0] == 0).all() and (want[3] == N.EMPTY).all()
    elif name == "an all-invalid map among others":
        assert not has[1].any() and has[0].any() and has[2].any() and (want[3][1] == N.EMPTY).all()
    elif name == "rectangles across the border":
        assert has.any() and (want[3][:, :, 0] != N.EMPTY).any() and ((want[0] != 0) & ~has).sum() > 100
    elif name == "rectangle wider than max_splat":
        full = N.ingest(*args, **dict(kw, max_splat=8))
        assert ((want[3] != N.EMPTY).sum() < (full[3] != N.EMPTY).sum())             # the cut leaves holes the full splat fills
    same(run(*args, **kw), want)


# ---- repeatability and reuse ------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits_and_out_is_the_fresh_path():
    name = "tile+1 3 views, colour 2.5x, C3 bilinear"
    args, kw, want = size_reference(name)
    a, b = run(*args, **kw), run(*args, **kw)
    same(a, want)
    same(b, a)
    V, Hd, Wd = args[0].shape
    Hc, Wc = args[1].shape[1:3]
    out = (torch.full((V, Hd, Wd), 7.0, device="cuda"), torch.full((V, Hd, Wd, 4), 9, dtype=torch.uint8, device="cuda"),
           torch.full((V, Hd, Wd), 7.0, device="cuda"))
    ws = kernels.rgbd_ingest_workspace(V, Hc, Wc)
    ws.fill_(12345)                                                 # a dirty workspace: the call clears the z-buffer itself
    v0 = [t._version for t in out]
    got = run(*args, out=out, workspace=ws, **kw)
    same(got, want)
    assert all(t._version > v for t, v in zip(out, v0))
    same(run(*args, out=out, workspace=ws, **kw), want)             # and again through the same buffers
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), bits(want[0]))
    # color_depth is optional; a wrong shape is refused
    got = run(*args, out=(out[0], out[1], None), workspace=ws, **kw)
    assert got[2] is None
    same(got[:2] + (want[2], got[3]), want)
    with pytest.raises(ValueError):
        run(*args, out=(out[0][:1], out[1], out[2]), **kw)
    with pytest.raises(ValueError):
        run(*args, workspace=ws[:16], **kw)


# ---- the hooks --------------------------------------------------------------------------------------------------------------------
def calibrations(views):
    return [RGBDCalibration(*v) for v in views]


def test_rgbd_ingest_over_17_views_equals_two_calls():
    raw, img, views, out_k = C.random_frame(17, 17, (6, 11), (9, 16), C=3)
    ing = RGBDIngest(calibrations(views), (6, 11), (9, 16), out_k)
    d, c, cd = ing(list(raw), list(img))
    torch.cuda.synchronize()
    kw = dict(sample=1, occl_tol=DEFAULT_OCCL_TOL, max_splat=8)
    first, last = run(raw[:16], img[:16], views[:16], out_k, **kw), run(raw[16:], img[16:], views[16:], out_k, **kw)
    for got, a, b in ((d, first[0], last[0]), (c, first[1], last[1]), (cd, first[2], last[2])):
        assert tuple(got.shape)[0] == 17
        g = got.cpu().numpy()
        assert np.array_equal(bits(g[:16]) if g.dtype == np.float32 else g[:16], bits(a) if a.dtype == np.float32 else a)
        assert np.array_equal(bits(g[16:]) if g.dtype == np.float32 else g[16:], bits(b) if b.dtype == np.float32 else b)
    same((d.cpu().numpy(), c.cpu().numpy(), cd.cpu().numpy(), None), N.ingest(raw, img, views, out_k, **kw)[:3] + (None,))
    # depth only
    d2, c2, cd2 = ing(list(raw))
    assert c2 is None and cd2 is None and torch.equal(d2, d)


R, NODES = 32, 64
H, W = 37, 53
ANGLES = (0.0, 40.0)


def raw_frames():
    """Frame 0 builds the canonical volume, frames 1 and 2 follow the moving sphere: per frame and view a raw uint16 depth map
    (millimetres, through the loop's own pinhole) and a raw colour image of twice the size from a camera 3 cm to the side."""
    K = DC.small_camera()
    scale = scene.grid_params(R)[0]
    lws = [scene.view_extrinsic(a) for a in ANGLES]
    rng = np.random.default_rng(19)
    depth, color = [], []
    for f in range(3):
        off = np.array([0.4, -0.25, 0.15]) * np.sin(0.5 * f) * scale
        maps = [scene.render_depth(K, lw, H, W, dtype=np.float64, invalid_frac=0.02, seed=11 + f, sphere_offset=off) for lw in lws]
        depth.append([np.rint(-m / 1e-3).astype(np.uint16) for m in maps])
        color.append([rng.integers(0, 256, size=(2 * H, 2 * W, 3), dtype=np.uint8) for _ in lws])
    k4 = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    T = np.hstack([np.eye(3), np.array([[-0.03], [0.0], [0.0]])])
    cal = [RGBDCalibration(k4, None, (2 * k4[0], 2 * k4[1], 2 * k4[2] + 0.5, 2 * k4[3] + 0.5), None, T) for _ in lws]
    return K, lws, depth, color, RGBDIngest(cal, (H, W), (2 * H, 2 * W), k4)


def new_loop(K, lws, first, ingest=None, **kw):
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(NODES, R)
    sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=2.0, distributed=False,
                   color_band=1.5, ingest=ingest, **kw)
    if ingest is not None:
        sf.integrate(first, lws)
    else:
        for d, lw in zip(first, lws):
            sf.integrate(d, lw)
    assert sf.refresh_samples() > 100
    return sf


@pytest.mark.parametrize("update", ["volume", "depth"])
def test_slab_frame_ingests_its_frames(update, monkeypatch):
    """SlabFrame(ingest=) on raw frames equals the stage called by hand in front of a SlabFrame without it: the depth maps to
    integrate() and step(), and the registered colours with the colour-only depth maps to the colour fusion, which the hand-made
    loop issues itself right after step() (relax = 1: the field the update used is still the solver's).  Volumes, colour volume
    and warp field agree bit for bit.  A third loop with ingest=None on the same pre-ingested maps never calls the stage."""
    K, lws, depth, color, ing = raw_frames()
    with pytest.raises(ValueError, match="ingest.K"):
        new_loop(K * np.array([[1.5], [1.0], [1.0]]), lws, depth[0], ingest=ing)
    a = new_loop(K, lws, depth[0], ingest=ing)
    d0 = [d.clone() for d in ing.frame(depth[0])[0]]
    b = new_loop(K, lws, d0)
    assert torch.equal(a.T, b.T) and torch.equal(a.Wt, b.Wt) and float(a.Wt.max()) > 0
    for ds, cs in zip(depth[1:], color[1:]):
        na = a.step(ds, lws, gn_iters=3, update=update, colors=cs, relax=1.0)
        dd, cc, cd = (list(t) for t in ing.frame(ds, cs))
        assert all(torch.equal(x, y) for x, y in zip(a.ingest_depth, dd)) and torch.equal(a.ingest_color, torch.stack(cc))
        assert torch.equal(a.color_depth, torch.stack(cd))
        dropped = (torch.stack(dd) != 0) & (torch.stack(cd) == 0)
        assert bool(dropped.any()) and bool((torch.stack(cd) != 0).any())                     # (pixels without a colour do exist)
        nb = b.step(dd, lws, gn_iters=3, update=update, relax=1.0)
        sv = b.fs.solver
        kernels.integrate_color(b.C, b.T, b.Wt, cd, cc, b.K, b.Kinv, lws, b.scale, b.center, b.tdist_world, b.color_band, sv.node_pos,
                                sv.node_dq, sv.node_w, b.knn, b.ident_lw, tsdf_res=R, res=(R, R, R), x_range=(b.a, b.b),
                                workspace=b.ws_dqb,
                                stored_indices=kernels.dqb_has_indices(b.ws_dqb, (R, R, R), b.knn, int(sv.node_pos.shape[0]), (b.a, b.b)))
        assert na == nb > 100
    torch.cuda.synchronize()
    assert torch.equal(a.T, b.T) and torch.equal(a.Wt, b.Wt) and torch.equal(a.fs.solver.node_dq, b.fs.solver.node_dq)
    assert torch.equal(a.C, b.C) and float(a.C[..., 3].max()) > 0
    # ingest=None: the calls it always issued -- the stage is never reached, and an explicit None equals the default
    def boom(*args, **kwargs):
        raise AssertionError("the ingest stage ran in a loop without one")
    monkeypatch.setattr(kernels, "rgbd_ingest", boom)
    c, d = new_loop(K, lws, d0, ingest=None), new_loop(K, lws, d0)
    for ds in depth[1:]:
        dd = [(-(torch.from_numpy(r.astype(np.float64)) * 1e-3)).float().cuda() for r in ds]
        assert c.step(dd, lws, gn_iters=3, update=update) == d.step(dd, lws, gn_iters=3, update=update)
    assert c.ingest is None and c.ingest_depth is None and c.color_depth is None
    assert torch.equal(c.T, d.T) and torch.equal(c.Wt, d.Wt) and torch.equal(c.fs.solver.node_dq, d.fs.solver.node_dq)


def test_fusion_dm_ingests_its_maps():
    """FusionDM.ingest: compute_live_tsdf(colors=) on raw frames equals the same call on the stage's depth maps, with the colour
    fusion issued by hand on the colour-only maps."""
    K, lws, depth, color, ing = raw_frames()
    tdist = scene.grid_params(R)[2]
    a, b = FusionDM(tdist, K, tsdf_res=R), FusionDM(tdist, K, tsdf_res=R)
    a.ingest = ing
    Ta, Wa = a.compute_live_tsdf(depth[0], lws, UseAutoAlignment=True, as_numpy=False, colors=color[0])
    dd, cc, cd = ing.frame(depth[0], color[0])
    Tb, Wb = b.compute_live_tsdf(dd, lws, UseAutoAlignment=True, as_numpy=False, colors=cc)
    assert torch.equal(Ta, Tb) and torch.equal(Wa, Wb) and float(Wa.max()) > 0
    assert a._C is not None and float(a._C[..., 3].max()) > 0
    assert bool((a._C[..., 3] <= b._C[..., 3]).all()) and not torch.equal(a._C, b._C)        # the colour-only maps let less in
    c = FusionDM(tdist, K * np.array([[1.5], [1.0], [1.0]]), tsdf_res=R)
    c.ingest = ing
    with pytest.raises(ValueError, match="ingest.K"):
        c.compute_live_tsdf(depth[0], lws, as_numpy=False)


def test_fusion_ingests_its_maps():
    """Fusion.ingest: InitializeCanonicalSpace(depths=, colors=) and updateTSDF_depths(colors=) on raw frames equal the same calls
    on the stage's depth maps, the colour fusion issued by hand on the colour-only maps."""
    from dynamicfusion_body_amd import Fusion
    K, lws, depth, color, ing = raw_frames()
    scale, center, tdist = scene.grid_params(R)
    a = Fusion(np.zeros((4, 4, 4)), tdist, subsample_rate=2.0, knn=2, write_warpfield=False)
    b = Fusion(np.zeros((4, 4, 4)), tdist, subsample_rate=2.0, knn=2, write_warpfield=False)
    a.ingest = ing
    a.InitializeCanonicalSpace(depths=depth[0], lws=lws, K=K, tsdf_size=R, scale=scale, center=center, colors=color[0])
    dd, cc, cd = ([t.clone() for t in ts] for ts in ing.frame(depth[0], color[0]))
    b.InitializeCanonicalSpace(depths=dd, lws=lws, K=K, tsdf_size=R, scale=scale, center=center)
    assert torch.equal(a._T, b._T) and torch.equal(a._Wt, b._Wt) and float(a._Wt.max()) > 0
    C = kernels.color_volume((R, R, R))
    kernels.integrate_color(C, b._T, b._Wt, cd, cc, K, np.linalg.inv(K), lws, scale, center, tdist, 1.5)
    assert torch.equal(a._C, C) and int((C[..., 3] > 0).sum()) > 100
    w0 = a._C[..., 3].clone()
    a.updateTSDF_depths(depth[1], lws, scale=scale, center=center, colors=color[1])
    b.updateTSDF_depths(ing.frame(depth[1])[0], lws, scale=scale, center=center)
    assert torch.equal(a._T, b._T) and torch.equal(a._Wt, b._Wt)
    assert bool((a._C[..., 3] >= w0).all()) and bool((a._C[..., 3] > w0).any())
    c = Fusion(np.zeros((4, 4, 4)), tdist, subsample_rate=2.0, knn=2, write_warpfield=False)
    c.ingest = ing
    with pytest.raises(ValueError, match="ingest.K"):
        c.InitializeCanonicalSpace(depths=depth[0], lws=lws, K=K * np.array([[1.5], [1.0], [1.0]]), tsdf_size=R, scale=scale, center=center)
