"""GPU: the visible-surface samples (csrc/dfh_render.hip dfh_render_samples_*, mesh.render_samples) against their numpy
restatement (tests/render_samples_np.py) bit for bit, against the resolve pass of the same raster, and as the sample source of
the frame loop (SlabFrame.visible_samples / set_sample_source) on the fixtures of tests/test_gpu_render.py."""
import functools

import numpy as np
import pytest
import torch

import render_np as RN
import render_samples_np as RS
from dynamicfusion_body_amd import _lib, mesh, scene
from dynamicfusion_body_amd.device import HostScalar, current_stream_ptr
from dynamicfusion_body_amd.pipeline import SlabFrame

pytestmark = pytest.mark.gpu

# constants of csrc/dfh_render.hip: lattice pixels per workgroup of the count / compact passes, counts per scan workgroup
SAMPLES_PIX, SAMPLES_CHUNK = 1024, 1024

HS, WS = 45, 67                                                          # neither a multiple of the strides 2 and 3
KS = scene.intrinsics(60.0, 33.2, 21.7)
SOUP_VIEWS = [scene.view_extrinsic(a) for a in (0.0, 25.0, -35.0)]
SCALE, HALF, CTR = 1.0 / 64, 32.0, np.array([0.0, 0.0, 2.0])
GEOM = dict(scale=SCALE, center=CTR, half=HALF)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _soup():
    """About 30 voxel-space triangles (world = (p - 32) / 64 + (0, 0, 2)) with every case the passes must get right, and
    canonical attributes that have nothing to do with the vertices.  Returns (verts, faces, canon_pos, canon_nrm)."""
    rng = np.random.default_rng(17)
    Wt = []
    for _ in range(12):                                              # random small / medium triangles
        c = CTR + rng.uniform(-0.4, 0.4, 3)
        Wt.append(c + rng.uniform(-0.15, 0.15, (3, 3)))
    for _ in range(3):                                               # quads: two triangles with an exact shared edge
        c = CTR + rng.uniform(-0.3, 0.3, 3)
        a, b = rng.uniform(-0.2, 0.2, 3), rng.uniform(-0.2, 0.2, 3)
        q = [c, c + a, c + a + b, c + b]
        Wt += [np.array([q[0], q[1], q[2]]), np.array([q[0], q[2], q[3]])]
    t = Wt[0]
    Wt.append(t.copy())                                              # an exact duplicate (the lower face id wins)
    Wt.append(t[[0, 2, 1]].copy())                                   # the same triangle, opposite winding
    Wt.append(np.array([t[0], t[0], t[1]]))                          # degenerate: repeated vertex
    Wt.append(np.array([t[0], 0.5 * (t[0] + t[1]), t[1]]))           # degenerate: collinear
    Wt.append(np.array([[0.0, 0.0, -1.0], [0.2, 0.0, -1.2], [0.0, 0.2, -1.1]]))   # behind every camera
    Wt.append(np.array([[0.0, 0.0, -0.5], [0.1, 0.1, 1.8], [-0.1, 0.1, 1.9]]))    # crosses the camera plane
    Wt.append(np.array([[0.5, 0.1, 2.0], [3.0, 0.2, 2.1], [0.6, 0.3, 2.2]]))      # partly off-screen (right)
    Wt.append(np.array([[-0.2, -2.5, 2.3], [0.1, -0.4, 2.0], [-0.3, -0.3, 2.1]])) # partly off-screen (top)
    Wt.append(np.array([[-6.0, -6.0, 3.5], [6.0, -6.0, 3.5], [0.0, 8.0, 3.5]]))   # covers the whole image of every view
    tris = np.array(Wt)
    verts = (tris.reshape(-1, 3) - CTR) / SCALE + HALF
    faces = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    cpos = rng.uniform(-50.0, 50.0, verts.shape)
    cnrm = rng.normal(size=verts.shape)
    return verts, faces, cpos, cnrm


@functools.lru_cache(maxsize=None)
def _soup_ref(stride):
    """The restatement's (pos, nrm, pixel) of the soup in the three views; computed once per stride and left unchanged."""
    verts, faces, cpos, cnrm = _soup()
    out = RS.render_samples(verts, faces, cpos, cnrm, KS, SOUP_VIEWS, HS, WS, stride=stride, face_map=_soup_faces(), **GEOM)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _soup_faces():
    verts, faces, _, _ = _soup()
    return RN.render(verts, faces, None, KS, SOUP_VIEWS, HS, WS, **GEOM)[2]


def _same(got, ref):
    pos, nrm, pix = (None if x is None else x.cpu().numpy() for x in got)
    rp, rn, rpix = ref
    assert pix.shape == rpix.shape, "count %d, restatement %d" % (len(pix), len(rpix))
    assert np.array_equal(pix, rpix)
    assert np.array_equal(_bits(pos), _bits(rp)), "pos differs in %d rows" % int((_bits(pos) != _bits(rp)).any(axis=1).sum())
    if rn is None:
        assert nrm is None
    else:
        assert np.array_equal(_bits(nrm), _bits(rn)), "nrm differs in %d rows" % int((_bits(nrm) != _bits(rn)).any(axis=1).sum())


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_soup_matches_restatement_bit_for_bit(stride):
    verts, faces, cpos, cnrm = _soup()
    assert len(faces) == 27
    ref = _soup_ref(stride)
    got = mesh.render_samples(verts, faces, cpos, cnrm, KS, SOUP_VIEWS, HS, WS, stride=stride, **GEOM)
    print("stride %d: %d samples of %d lattice pixels" % (stride, len(ref[2]), 3 * len(range(0, HS, stride)) * len(range(0, WS, stride))))
    _same(got, ref)
    # the whole-image triangle: every lattice pixel of view 0 is a sample; several faces are seen; the duplicate never wins
    fm = _soup_faces()
    assert np.all(fm[0] >= 0) and len(np.unique(fm)) > 10 and not np.any(fm == 18)
    assert len(ref[2]) >= len(range(0, HS, stride)) * len(range(0, WS, stride))
    # batched against per-view calls
    hw = HS * WS
    for v, lw in enumerate(SOUP_VIEWS):
        one = mesh.render_samples(verts, faces, cpos, cnrm, KS, lw, HS, WS, stride=stride, **GEOM)
        sel = (got[2] >= v * hw) & (got[2] < (v + 1) * hw)
        assert torch.equal(one[2] + v * hw, got[2][sel]) and torch.equal(one[0], got[0][sel]) and torch.equal(one[1], got[1][sel])
    # numpy inputs and CUDA inputs; no canonical normals -> no normal output, the same positions
    cu = lambda a: torch.from_numpy(np.array(a)).cuda()
    p2, n2, x2 = mesh.render_samples(cu(verts), cu(faces), cu(cpos), None, KS, SOUP_VIEWS, HS, WS, stride=stride, **GEOM)
    assert n2 is None and torch.equal(p2, got[0]) and torch.equal(x2, got[2])


def test_deterministic():
    verts, faces, cpos, cnrm = _soup()
    a = mesh.render_samples(verts, faces, cpos, cnrm, KS, SOUP_VIEWS, HS, WS, stride=2, **GEOM)
    b = mesh.render_samples(verts, faces, cpos, cnrm, KS, SOUP_VIEWS, HS, WS, stride=2, **GEOM)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _raw(verts, faces, cpos, cnrm, K, lws, H, W, stride, capacity, rows):
    """The three library calls of mesh.render_samples with the emit's capacity chosen freely and `rows` output rows
    pre-filled with a pattern: (total, pos, nrm, pixel)."""
    lib = _lib.load()
    Kf, lwf, nv = mesh._view_table(K, lws)
    dev = "cuda"
    V, P, N = (torch.from_numpy(np.array(a, dtype=np.float64)).to(dev) for a in (verts, cpos, cnrm))
    F = torch.from_numpy(np.array(faces, dtype=np.int32)).to(dev)
    wsp = mesh.render_workspace(nv, H, W, F.shape[0], dev)
    Ka, La, Ca = _lib.darr(Kf, 9 * nv), _lib.darr(lwf, 12 * nv), _lib.darr(CTR, 3)
    ws, nbytes = wsp.buf.data_ptr(), wsp.buf.numel() * 8
    st = current_stream_ptr()
    _lib.check(lib.dfh_render_raster(V.data_ptr(), V.shape[0], F.data_ptr(), F.shape[0], nv, Ka, La, H, W, SCALE, Ca, HALF, 1e-3, ws, nbytes, st),
               "dfh_render_raster")
    sbytes = lib.dfh_render_samples_workspace_bytes(nv, H, W, stride)
    scan = torch.empty((sbytes + 7) // 8, dtype=torch.int64, device=dev)
    total = HostScalar(torch.int64)
    _lib.check(lib.dfh_render_samples_count(nv, H, W, F.shape[0], stride, ws, nbytes, scan.data_ptr(), scan.numel() * 8, total.ptr(), st),
               "dfh_render_samples_count")
    n = total.get()
    pos = torch.full((rows, 3), 7.5, dtype=torch.float64, device=dev)
    nrm = torch.full((rows, 3), 7.5, dtype=torch.float64, device=dev)
    pix = torch.full((rows,), -7, dtype=torch.int64, device=dev)
    _lib.check(lib.dfh_render_samples_emit(V.data_ptr(), P.data_ptr(), N.data_ptr(), V.shape[0], F.data_ptr(), F.shape[0], nv, Ka, La, H, W,
                                           SCALE, Ca, HALF, 1e-3, stride, ws, nbytes, scan.data_ptr(), scan.numel() * 8, pos.data_ptr(),
                                           nrm.data_ptr(), pix.data_ptr(), capacity, st), "dfh_render_samples_emit")
    torch.cuda.synchronize()
    return n, pos.cpu().numpy(), nrm.cpu().numpy(), pix.cpu().numpy()


def test_capacity_gives_the_even_subsample_and_writes_no_row_beyond_the_count():
    verts, faces, cpos, cnrm = _soup()
    rp, rn, rpix = _soup_ref(2)
    total = len(rpix)
    assert total > 100
    for cap in (0, 1, total - 1, total, total + 5, total // 3):
        n, pos, nrm, pix = _raw(verts, faces, cpos, cnrm, KS, SOUP_VIEWS, HS, WS, 2, cap, total + 8)
        assert n == total
        keep = RS.subsample_index(total, cap)
        m = min(cap, total)
        assert len(keep) == m
        assert np.array_equal(pix[:m], rpix[keep]) and np.array_equal(_bits(pos[:m]), _bits(rp[keep])) \
            and np.array_equal(_bits(nrm[:m]), _bits(rn[keep])), cap
        assert np.all(pix[m:] == -7) and np.all(pos[m:] == 7.5) and np.all(nrm[m:] == 7.5), cap
    # the Python entry point: max_samples
    got = mesh.render_samples(verts, faces, cpos, cnrm, KS, SOUP_VIEWS, HS, WS, stride=2, max_samples=total // 3, **GEOM)
    keep = RS.subsample_index(total, total // 3)
    _same(got, (rp[keep], rn[keep], rpix[keep]))
    assert mesh.render_samples(verts, faces, cpos, cnrm, KS, SOUP_VIEWS, HS, WS, stride=2, max_samples=total + 5, **GEOM)[2].shape[0] == total


def test_empty_cases_give_count_zero():
    verts, faces, cpos, cnrm = _soup()
    pos, nrm, pix = mesh.render_samples(verts, np.zeros((0, 3), dtype=np.int32), cpos, cnrm, KS, SOUP_VIEWS, HS, WS, **GEOM)
    assert pos.shape == (0, 3) and nrm.shape == (0, 3) and pix.shape == (0,) and pix.dtype == torch.int64
    pos, nrm, pix = mesh.render_samples(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int32), np.zeros((0, 3)), None, KS, SOUP_VIEWS, HS, WS)
    assert pos.shape == (0, 3) and nrm is None and pix.shape == (0,)
    behind = faces[[20, 21, 22, 23]]                                  # degenerate, behind every camera, across the camera plane
    n, pos, nrm, pix = _raw(verts, behind, cpos, cnrm, KS, SOUP_VIEWS, HS, WS, 1, 4, 4)
    assert n == 0 and np.all(pix == -7) and np.all(pos == 7.5) and np.all(nrm == 7.5)
    assert mesh.render_samples(verts, behind, cpos, cnrm, KS, SOUP_VIEWS, HS, WS, **GEOM)[0].shape == (0, 3)


def test_scan_boundaries_whole_images():
    """One triangle that covers every pixel of every view, at a size that crosses a workgroup boundary of the count pass
    (SAMPLES_PIX lattice pixels), a chunk boundary of the scan (SAMPLES_CHUNK workgroups) and ends inside a workgroup: with
    stride 1 every pixel is a sample, in order; with stride 3 (workgroup boundaries only: sixteen views of this size stay
    inside one chunk) every lattice pixel."""
    V, H, W = 5, 419, 503
    assert V * H * W > SAMPLES_PIX * SAMPLES_CHUNK and (V * H * W) % SAMPLES_PIX != 0
    K = scene.intrinsics(400.0, 251.3, 209.6)
    lw = scene.view_extrinsic(0.0)
    tri = (np.array([[-6.0, -6.0, 3.5], [6.0, -6.0, 3.5], [0.0, 8.0, 3.5]]) - CTR) / SCALE + HALF
    faces = np.array([[0, 1, 2]], dtype=np.int32)
    pos, nrm, pix = mesh.render_samples(tri, faces, tri, None, K, [lw] * V, H, W, **GEOM)
    assert pix.shape[0] == V * H * W and torch.equal(pix, torch.arange(V * H * W, device="cuda"))
    # canon_pos = verts: every sample lies on the plane z_world = 3.5 and projects onto its own pixel
    P = (pos - HALF) * SCALE + torch.from_numpy(CTR).cuda()
    cam = P @ torch.from_numpy(lw[:, :3].T.copy()).cuda() + torch.from_numpy(lw[:, 3].copy()).cuda()
    u = (K[0, 0] * cam[:, 0] + K[0, 2] * cam[:, 2]) / cam[:, 2]
    v = (K[1, 1] * cam[:, 1] + K[1, 2] * cam[:, 2]) / cam[:, 2]
    rem = pix % (H * W)
    assert float((u - (rem % W)).abs().max()) <= 1e-9 and float((v - (rem // W)).abs().max()) <= 1e-9
    assert float((P[:, 2] - 3.5).abs().max()) <= 1e-12
    V3 = V
    Hs, Ws = len(range(0, H, 3)), len(range(0, W, 3))
    pos3, _, pix3 = mesh.render_samples(tri, faces, tri, None, K, [lw] * V3, H, W, stride=3, **GEOM)
    want = (torch.arange(V3, device="cuda")[:, None, None] * H + 3 * torch.arange(Hs, device="cuda")[None, :, None]) * W \
        + 3 * torch.arange(Ws, device="cuda")[None, None, :]
    assert torch.equal(pix3, want.reshape(-1))
    first = pix[:H * W]
    assert torch.equal(pos3[:Hs * Ws], pos[:H * W][((first // W) % 3 == 0) & ((first % W) % 3 == 0)])


@pytest.mark.parametrize("stride", [1, 2])
def test_agrees_with_the_resolve_pass(stride):
    """The samples' pixels are the lattice pixels that mesh.render's face map covers; with canon_pos = verts a sample is the
    surface point of its pixel: it projects onto the pixel's centre, at the depth the resolve pass stores."""
    verts, faces, _, cnrm = _soup()
    depth, _, face = mesh.render(verts, faces, None, KS, SOUP_VIEWS, HS, WS, **GEOM)
    pos, nrm, pix = mesh.render_samples(verts, faces, verts, cnrm, KS, SOUP_VIEWS, HS, WS, stride=stride, **GEOM)
    lattice = torch.zeros((3, HS, WS), dtype=torch.bool, device="cuda")
    lattice[:, ::stride, ::stride] = True
    assert torch.equal(pix, torch.nonzero((lattice & (face >= 0)).reshape(-1))[:, 0])
    pos, pix, depth = pos.cpu().numpy(), pix.cpu().numpy(), depth.cpu().numpy().reshape(-1)
    hw = HS * WS
    for v, lw in enumerate(SOUP_VIEWS):
        sel = pix // hw == v
        u, vv, z = RN.project(pos[sel], KS, lw, SCALE, CTR, HALF)
        rem = pix[sel] % hw
        assert np.abs(u - rem % WS).max() <= 1e-9 and np.abs(vv - rem // WS).max() <= 1e-9
        assert np.array_equal(z.astype(np.float32), -depth[pix[sel]])
    assert np.abs(np.linalg.norm(nrm.cpu().numpy(), axis=1) - 1.0).max() <= 1e-15 * 4


def test_bad_arguments_raise():
    verts, faces, cpos, cnrm = _soup()
    for kw in (dict(stride=0), dict(stride=-1), dict(max_samples=-1)):
        with pytest.raises(ValueError):
            mesh.render_samples(verts, faces, cpos, cnrm, KS, SOUP_VIEWS, HS, WS, **kw)
    with pytest.raises(ValueError):
        mesh.render_samples(verts, faces, cpos[:-1], cnrm, KS, SOUP_VIEWS, HS, WS)
    with pytest.raises(ValueError):
        mesh.render_samples(verts, faces, cpos, cnrm[:, :2], KS, SOUP_VIEWS, HS, WS)
    with pytest.raises(ValueError):
        mesh.render_samples(verts, faces, cpos, cnrm, np.eye(4), SOUP_VIEWS, HS, WS)
    with pytest.raises(ValueError):
        mesh.render_samples(verts, faces, cpos, cnrm, KS, [SOUP_VIEWS[0]] * 17, HS, WS)


# ---- the frame loop: fixtures of tests/test_gpu_render.py (128^3, 256 nodes, two views of camera C1) -------------------------
H1, W1, F1, CX1, CY1 = scene.CAMERAS["C1"]
K1 = scene.intrinsics(F1, CX1, CY1)
R = 128
VIEWS = [scene.view_extrinsic(0.0), scene.view_extrinsic(120.0)]


@functools.lru_cache(maxsize=None)
def _observed(lw_key, offset_key):
    """The analytic depth map of the sphere (moved by `offset` metres) in one view; computed once per view and offset."""
    lw = np.array(lw_key).reshape(3, 4)
    off = None if offset_key is None else np.array(offset_key)
    d = scene.render_depth(K1, lw, H1, W1, dtype=np.float32, invalid_frac=0.0, wall_z=None, sphere_offset=off)
    d.setflags(write=False)
    return d


def _obs(lw, offset=None):
    return _observed(tuple(np.asarray(lw).reshape(-1)), None if offset is None else tuple(offset))


def _static_frame(n_nodes=256, keep_nodes=None):
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(n_nodes, R)
    if keep_nodes is not None:
        node_pos, node_w = node_pos[:keep_nodes], node_w[:keep_nodes]
    sf = SlabFrame(K1, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=2.0, distributed=False)
    for lw in [scene.view_extrinsic(45.0 * v) for v in range(8)]:
        sf.integrate(torch.from_numpy(np.array(_obs(lw))).cuda(), lw)
    sf.refresh_samples()
    return sf, scale


def _depths(offset=None):
    return [torch.from_numpy(np.array(_obs(lw, offset))).cuda() for lw in VIEWS]


def _frame_error(sf, offset, scale):
    depth, _, _ = sf.render_live(VIEWS, H1, W1)
    obs = np.stack([_obs(lw, offset) for lw in VIEWS])
    errs = mesh.depth_error(depth, torch.from_numpy(obs).cuda(), 0.5 * scale)
    d = depth.cpu().numpy()
    cover = [float(((d[v] != 0) & (obs[v] != 0)).sum()) / float((obs[v] != 0).sum()) for v in range(len(VIEWS))]
    return errs, cover


def test_slab_frame_visible_source_counts_the_covered_lattice_pixels():
    sf, _ = _static_frame()
    n_band = sf.fs.solver.S
    _, _, face = sf.render_live(VIEWS, H1, W1)
    for stride in (1, 2):
        sf.set_sample_source("visible", VIEWS, (H1, W1), stride=stride)
        want = int((face[:, ::stride, ::stride] >= 0).sum())
        assert sf.fs.solver.S == want > 1000
        pos, nrm, pix = sf.visible_samples(VIEWS, H1, W1, stride=stride)
        assert pos.shape == (want, 3) and nrm.shape == (want, 3) and pix.shape == (want,)
        if stride == 1:
            assert torch.equal(pix, torch.nonzero(face.reshape(-1) >= 0)[:, 0])
        # canonical points on the sphere's zero level set (radius 0.5 m about the grid centre), unit normals
        r = (pos - R / 2).norm(dim=1) * scene.GRID_SIDE / R
        assert float((r - scene.SPHERE_R).abs().max()) <= 1.0 * scene.GRID_SIDE / R
        assert float((nrm.norm(dim=1) - 1.0).abs().max()) <= 1e-12
        assert sf.refresh_samples() == want
    sf.set_sample_source("visible", VIEWS, (H1, W1), max_samples=5000)
    assert sf.fs.solver.S == 5000
    sf.set_sample_source("band")
    assert sf.fs.solver.S == n_band


def test_slab_frame_visible_source_static_sphere():
    """tests/test_gpu_render.py's static-sphere check with the rendered model as the sample source: after three steps the
    rendered live model lies within half a voxel (median) of the observed frame on 95 % of its pixels."""
    sf, scale = _static_frame()
    sf.set_sample_source("visible", VIEWS, (H1, W1))
    for _ in range(3):
        n = sf.step(_depths(), VIEWS, gn_iters=5)
        assert n == sf.fs.solver.S > 1000
    errs, cover = _frame_error(sf, None, scale)
    print("static sphere, visible source, render_live vs observed:", [(e["median"] / scale, e["n_within"] / max(e["n_valid"], 1)) for e in errs], cover)
    for e, c in zip(errs, cover):
        assert e["median"] <= 0.5 * scale and c >= 0.95


def test_slab_frame_moving_sequence_band_and_visible():
    """The ten-frame moving sequence of tests/test_gpu_render.py under both sample sources in one run: the visible loop's
    worst per-frame median |rendered - observed| is at most twice the band loop's (the margin that test grants the sequence)."""
    amp = np.array([0.8, -0.5, 0.4])
    med = {}
    for source in ("band", "visible"):
        sf, scale = _static_frame()
        if source == "visible":
            sf.set_sample_source("visible", VIEWS, (H1, W1))
        med[source] = []
        for t in range(10):
            off = amp * np.sin(2 * np.pi * (t + 1) / 30.0) * scale
            sf.step(_depths(off), VIEWS, gn_iters=10)
            errs, cover = _frame_error(sf, off, scale)
            med[source].append(max(e["median"] for e in errs) / scale)
            assert min(cover) >= 0.95
        print("moving sequence, %s source (S = %d): per-frame median |rendered - observed| (voxels, worst view): %s"
              % (source, sf.fs.solver.S, [round(m, 4) for m in med[source]]))
    assert max(med["visible"]) <= 2 * max(med["band"])


def test_update_graph_inserts_the_same_nodes_under_either_source():
    """Graph growth reads the band samples whatever the source: from identical states (a graph that supports only part of the
    sphere) both sources insert the same nodes."""
    a, _ = _static_frame(keep_nodes=96)
    b, _ = _static_frame(keep_nodes=96)
    b.set_sample_source("visible", VIEWS, (H1, W1), stride=2)
    na, nb = a.update_graph(), b.update_graph()
    assert na == nb > 0
    assert torch.equal(a.fs.solver.node_pos, b.fs.solver.node_pos) and torch.equal(a.fs.solver.node_dq, b.fs.solver.node_dq)
    assert torch.equal(a.fs.solver.node_w, b.fs.solver.node_w)
    assert a.sample_source == "band" and b.sample_source == "visible" and 0 < b.fs.solver.S < a.fs.solver.S


def test_set_sample_source_refuses_bad_arguments():
    scale, center, tdist = scene.grid_params(32)
    node_pos, node_w = scene.fibonacci_nodes(16, 32)
    sf = SlabFrame(K1, scale, center, 32, tdist / scale, node_pos, node_w, knn=4, distributed=False)
    with pytest.raises(ValueError):
        sf.set_sample_source("mesh")
    with pytest.raises(ValueError):
        sf.set_sample_source("visible")
    with pytest.raises(ValueError):
        sf.set_sample_source("visible", VIEWS)
    with pytest.raises(ValueError):
        sf.set_sample_source("visible", size=(H1, W1))
    with pytest.raises(ValueError):
        sf.set_sample_source("visible", VIEWS, (H1, W1), stride=0)
    with pytest.raises(ValueError):
        sf.set_sample_source("band", stride=0)
    assert sf.sample_source == "band"
    # an empty volume: nothing visible is a valid state
    sf.set_sample_source("visible", VIEWS, (H1, W1))
    assert sf.fs.solver.S == 0 and sf.refresh_samples() == 0
    sf.set_sample_source("band")
    sf.ws = 2                                                         # what a two-rank job's frame looks like to the methods
    with pytest.raises(ValueError):
        sf.set_sample_source("visible", VIEWS, (H1, W1))
    with pytest.raises(ValueError):
        sf.visible_samples(VIEWS, H1, W1)
    assert sf.sample_source == "band"


def test_pcg_timeout_surfaces_with_the_visible_source():
    """step() ends with the sample refresh, whose count read-back synchronises, and then asks check_status(completed_only):
    a persistent PCG solve that timed out in its grid barrier (forced by a spin bound of 0 polls, as in
    tests/test_gpu_solve.py) raises there with the visible source as it does with the band source."""
    lib = _lib.load()
    sf, _ = _static_frame()
    sf.set_sample_source("visible", VIEWS, (H1, W1), stride=2)
    lib.dfh_pcg_set_mode(0)
    try:
        assert sf.fs.solver.N > 8 and lib.dfh_pcg_path(sf.fs.solver.N) == 1      # the persistent kernel, a real grid barrier
        _lib.set_option("pcg_spin_limit", 0)
        with pytest.raises(_lib.DfhTimeout):
            sf.step(_depths(), VIEWS, gn_iters=2, global_iters=0)
        _lib.set_option("pcg_spin_limit", None)
        lib.dfh_pcg_set_mode(0)
        assert sf.step(_depths(), VIEWS, gn_iters=2) == sf.fs.solver.S > 1000       # the next frame is sound
        sf.fs.solver.check_status()
    finally:
        _lib.set_option("pcg_spin_limit", None)
        lib.dfh_pcg_set_mode(0)
