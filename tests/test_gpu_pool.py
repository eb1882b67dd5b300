"""GPU: K15 -- dfh_pool_features and dfh_render_vertex_ids against their numpy restatements (tests/pool_np.py), bit for bit; the
reference's golden pooled on the device; 24 views through the 16-view rasteriser; and the whole chain (regularise, render,
a feature function that back-projects every pixel, pool, nearest descriptor) on a sphere, where a vertex's descriptor must be
its own position."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pool_np as PN
from dynamicfusion_body_amd import Fusion, _lib, descriptors, mesh
from dynamicfusion_body_amd.device import current_stream_ptr

pytestmark = pytest.mark.gpu

# the kernels as built (dfh_pool_features_tile): the count and scatter passes take PIX pixels per workgroup, the scan SCAN
# vertices; a segment of up to CAP entries is ordered in LDS, a longer one by a walk over vid in steps of STEP pixels
PIX, SCAN, CAP, STEP = 256, 1024, 1024, 1024
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g10_pool.npz")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_tile_constants_are_the_kernels():
    tile = (ctypes.c_int * 4)()
    assert _lib.load().dfh_pool_features_tile(tile) == 0
    assert list(tile) == [PIX, SCAN, CAP, STEP]


def check(vid, feats, n_verts, what=None):
    """feat bit-equal and cnt equal to the restatement; returns the device's (feat, cnt) as numpy."""
    feat, cnt = descriptors.pool_features(vid, feats, n_verts)
    feat, cnt = feat.cpu().numpy(), cnt.cpu().numpy()
    rfeat, rcnt = PN.pool_features(vid, feats, n_verts)
    assert feat.dtype == np.float32 and cnt.dtype == np.int32 and feat.shape == rfeat.shape
    assert np.array_equal(cnt, rcnt), (what, np.flatnonzero(cnt != rcnt)[:8])
    assert np.array_equal(_bits(feat), _bits(rfeat)), (what, np.argwhere(_bits(feat) != _bits(rfeat))[:8])
    return feat, cnt


def wide(rng, shape):
    """float32 values over eleven decades: partial sums round, the order of the additions shows."""
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 8, size=shape)).astype(np.float32)


@pytest.mark.parametrize("dim", [1, 3, 16, 17, 64])
def test_sizes_at_the_kernels_edges(dim):
    rng = np.random.default_rng(200 + dim)
    sizes = [0, 1, 2]
    for t in sorted({PIX, SCAN, STEP}):
        sizes += [t - 1, t, t + 1]
    sizes += [3 * PIX + 7]
    for n_pixels in sizes:
        for n_verts in (1, 7, 300):
            vid = rng.integers(-1, n_verts, size=n_pixels).astype(np.int32)
            check(vid, wide(rng, (n_pixels, dim)), n_verts, (dim, n_pixels, n_verts))
    for n_verts in (SCAN - 1, SCAN, SCAN + 1, 2 * SCAN + 3):         # the scan's chunks; most vertices own one pixel or none
        vid = rng.integers(-1, n_verts, size=n_verts).astype(np.int32)
        _, cnt = check(vid, wide(rng, (n_verts, dim)), n_verts, (dim, "scan", n_verts))
        assert (cnt == 0).any() and (cnt > 1).any()


def test_more_scan_chunks_than_one_round_of_the_top_scan():
    """The scan of the chunk totals takes PIX chunks a round and carries their sum into the next: one chunk beyond a round."""
    rng = np.random.default_rng(77)
    n_verts = PIX * SCAN + 5
    vid = rng.integers(-1, n_verts, size=n_verts).astype(np.int32)
    vid[[3, n_verts // 2]] = n_verts - 1                               # a segment of the last chunk: it starts behind the carry
    _, cnt = check(vid, wide(rng, (n_verts, 1)), n_verts, ("top scan", n_verts))
    assert (cnt == 0).any() and (cnt > 1).any() and cnt[-1] >= 2


def test_ids_that_are_no_vertex():
    rng = np.random.default_rng(5)
    n, n_verts, dim = 3000, 40, 16
    feats = wide(rng, (n, dim))
    feat, cnt = check(np.full(n, -1, dtype=np.int32), feats, n_verts, "every id -1")
    assert (cnt == 0).all() and (_bits(feat) == 0).all()              # +0.0f, not -0.0f
    vid = rng.integers(0, n_verts, size=n).astype(np.int32)
    vid[::3] = n_verts                                                # one past the last vertex
    vid[1::7] = -2
    vid[2::11] = np.iinfo(np.int32).min
    vid[5::13] = np.iinfo(np.int32).max
    vid[vid == 17] = -1                                               # a vertex with no pixel
    feat, cnt = check(vid, feats, n_verts, "ids outside [0, n_verts)")
    assert cnt[17] == 0 and (_bits(feat[17]) == 0).all() and cnt.sum() == ((vid >= 0) & (vid < n_verts)).sum()
    # any shape of vid, CUDA tensors in place of numpy
    f2, c2 = descriptors.pool_features(torch.from_numpy(vid.reshape(3, 10, 100)).cuda(), torch.from_numpy(feats.reshape(3, 10, 100, dim)).cuda(),
                                       n_verts)
    assert np.array_equal(_bits(f2.cpu().numpy()), _bits(feat)) and np.array_equal(c2.cpu().numpy(), cnt)
    with pytest.raises(ValueError, match="shape of vid"):
        descriptors.pool_features(vid, feats.reshape(-1), n_verts)
    with pytest.raises(ValueError, match="channels"):
        descriptors.pool_features(vid, np.zeros((n, 65), dtype=np.float32), n_verts)


@pytest.mark.parametrize("dim", [3, 16])
def test_segments_at_the_lds_cap(dim):
    """Vertices owning CAP - 1, CAP and CAP + 1 pixels (the last takes the ordered walk), scattered among short segments."""
    rng = np.random.default_rng(9)
    lengths = {2: CAP - 1, 5: CAP, 11: CAP + 1, 12: 2 * CAP + 77, 30: 1, 31: 64, 32: 65}
    n_verts = 40
    vid = np.concatenate([np.full(n, v, dtype=np.int32) for v, n in lengths.items()] + [rng.integers(13, 30, size=900).astype(np.int32),
                                                                                      np.full(500, -1, dtype=np.int32)])
    rng.shuffle(vid)
    _, cnt = check(vid, wide(rng, (len(vid), dim)), n_verts, "cap")
    for v, n in lengths.items():
        assert cnt[v] == n


def test_one_vertex_owns_every_pixel():
    rng = np.random.default_rng(13)
    n = 70000
    for n_verts, v in ((1, 0), (5, 3)):
        feat, cnt = check(np.full(n, v, dtype=np.int32), wide(rng, (n, 16)), n_verts, "one vertex")
        assert cnt[v] == n and cnt.sum() == n


def test_the_order_decides_the_bits():
    """1e8, 1, -1e8 interleaved: ascending order gives (1e8 + 1) - 1e8 = 0 per triple, any other order something else."""
    n_verts, per = 50, 300
    rng = np.random.default_rng(17)
    vid = np.repeat(np.arange(n_verts, dtype=np.int32), per)
    rng.shuffle(vid)
    feats = np.tile(np.array([1e8, 1.0, -1e8], dtype=np.float32), len(vid) // 3)[:, None] * np.ones((1, 4), dtype=np.float32)
    feat, _ = check(vid, feats, n_verts, "1e8, 1, -1e8")
    down, _ = PN.pool_features(vid, feats, n_verts, descending=True)
    assert (_bits(down) != _bits(feat)).any()
    sums = np.unique(feat)
    assert len(sums) > 3                                              # the vertices' pixel sets differ, and so do their sums


def test_special_values():
    rng = np.random.default_rng(19)
    n, n_verts, dim = 4000, 30, 16
    vid = rng.integers(0, n_verts, size=n).astype(np.int32)
    feats = wide(rng, (n, dim))
    first = [np.flatnonzero(vid == v)[0] for v in range(8)]
    feats[first[0], 0] = np.nan
    feats[first[1], 1] = np.inf
    feats[first[2], 2] = -np.inf
    feats[first[3], 3] = np.inf
    feats[np.flatnonzero(vid == 3)[5], 3] = -np.inf                   # inf + -inf = NaN
    feats[vid == 4] = -0.0                                            # +0.0f + -0.0f = +0.0f
    feats[vid == 5] = np.float32(1e-41)                               # subnormals
    feats[vid == 6] = np.float32(3e38)                                # overflow to +inf on the way
    feats[first[7]] = np.float32(-1e-45)
    feat, cnt = check(vid, feats, n_verts, "special values")
    assert np.isnan(feat[0, 0]) and np.isposinf(feat[1, 1]) and np.isneginf(feat[2, 2]) and np.isnan(feat[3, 3])
    assert (_bits(feat[4]) == 0).all() and np.isposinf(feat[6]).all()
    assert (feat[5] > 0).all() and (feat[5] < np.finfo(np.float32).tiny).all()


def _raw_pool(vid, feats, n_verts, stream=None, guard=8):
    """The C entry point with guard words behind both outputs."""
    lib = _lib.load()
    n, dim = vid.numel(), feats.shape[-1]
    out = torch.full((n_verts * dim + guard,), -7.5, dtype=torch.float32, device="cuda")
    cnt = torch.full((n_verts + guard,), -12345, dtype=torch.int32, device="cuda")
    nbytes = lib.dfh_pool_features_workspace_bytes(n, n_verts)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device="cuda")
    _lib.check(lib.dfh_pool_features(vid.data_ptr(), feats.data_ptr(), n, dim, n_verts, out.data_ptr(), cnt.data_ptr(), ws.data_ptr(), nbytes,
                                     current_stream_ptr() if stream is None else stream.cuda_stream), "dfh_pool_features")
    return out, cnt


def test_determinism_containment_and_a_side_stream():
    rng = np.random.default_rng(23)
    n, n_verts, dim = 50000, 333, 16
    vn = rng.integers(-1, n_verts, size=n).astype(np.int32)
    vn[rng.random(n) < 0.1] = 7                                       # one long segment (the ordered walk)
    fn = wide(rng, (n, dim))
    vid, feats = torch.from_numpy(vn).cuda(), torch.from_numpy(fn).cuda()
    rfeat, rcnt = PN.pool_features(vn, fn, n_verts)
    assert rcnt[7] > CAP
    a = _raw_pool(vid, feats, n_verts)
    b = _raw_pool(vid, feats, n_verts)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = _raw_pool(vid, feats, n_verts, stream=side)
    side.synchronize()
    for x in (b, c):
        assert torch.equal(_as_int(a[0]), _as_int(x[0])) and torch.equal(a[1], x[1])
    out, cnt = a
    assert np.array_equal(_bits(out[:n_verts * dim].cpu().numpy().reshape(n_verts, dim)), _bits(rfeat))
    assert np.array_equal(cnt[:n_verts].cpu().numpy(), rcnt)
    assert (out[n_verts * dim:] == -7.5).all() and (cnt[n_verts:] == -12345).all()
    # no pixels: zeros and counts of zero are written; no vertices: nothing is
    out, cnt = _raw_pool(vid[:0], feats[:0], n_verts)
    assert (_as_int(out[:n_verts * dim]) == 0).all() and (cnt[:n_verts] == 0).all() and (out[n_verts * dim:] == -7.5).all()
    out, cnt = _raw_pool(vid, feats, 0)
    assert (out == -7.5).all() and (cnt == -12345).all()


def _as_int(t):
    return t.view(torch.int32)


def test_golden_on_the_device():
    g = np.load(GOLDEN)
    vid = np.stack([PN.golden_ids(v) for v in range(PN.G_VIEWS)])
    feats = np.stack([PN.golden_features(v) for v in range(PN.G_VIEWS)])
    feat, cnt = descriptors.pool_features(vid, feats, PN.G_VERTS)
    assert np.array_equal(_bits(feat.cpu().numpy()), _bits(g["feat"]))
    assert int(cnt.sum()) == int((vid >= 0).sum())


# ---- dfh_render_vertex_ids -------------------------------------------------------------------------------------------------------------
SH, SW = 45, 67
SK = np.array([[64.0, 0.0, 32.0], [0.0, 64.0, 16.0], [0.0, 0.0, 1.0]])
TIE_PIXELS = {(26, 14): 2, (26, 10): 1, (29, 16): 2, (23, 16): 2}    # (x, y) -> corner: centroid, midpoints of 01, 12, 02


def _turn_y(deg, pivot=(0.0, 0.0, 2.5)):
    a = np.radians(deg)
    Rm = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    p = np.asarray(pivot)
    return np.concatenate([Rm, (p - Rm @ p)[:, None]], axis=1)


SOUP_VIEWS = np.stack([_turn_y(0.0), _turn_y(20.0), _turn_y(-30.0)])


def _soup():
    """A small indexed triangle soup in camera-0 coordinates (scale 1, half 0, centre 0); returns (verts, faces, index of the tie
    triangle's first vertex)."""
    rng = np.random.default_rng(29)
    V, F = [], []

    def add(tri):
        F.append([len(V), len(V) + 1, len(V) + 2])
        V.extend(np.asarray(tri, dtype=np.float64))
    for _ in range(25):                                               # random triangles behind the tie triangle's depth
        c = np.array([rng.uniform(-0.7, 0.7), rng.uniform(-0.4, 0.6), rng.uniform(2.5, 3.2)])
        add(c + rng.uniform(-0.25, 0.25, (3, 3)))
    for _ in range(5):                                                # fans: four triangles around a shared centre vertex,
        c = np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.3, 0.5), rng.uniform(2.4, 3.0)])   # every edge shared
        ring = [c + np.array([0.2 * np.cos(t), 0.2 * np.sin(t), rng.uniform(-0.1, 0.1)]) for t in np.arange(4) * np.pi / 2 + 0.3]
        i0 = len(V)
        V.extend([c] + ring)
        F += [[i0, i0 + 1 + k, i0 + 1 + (k + 1) % 4] for k in range(4)]
    F.append(list(F[0]))                                              # an exact duplicate (the lower face id wins)
    F.append([F[1][0], F[1][2], F[1][1]])                             # the same triangle, opposite winding
    F.append([F[2][0], F[2][0], F[2][1]])                             # degenerate: repeated vertex
    add([V[F[3][0]], 0.5 * (V[F[3][0]] + V[F[3][1]]), V[F[3][1]]])    # degenerate: collinear
    add([[0.0, 0.0, -1.0], [0.2, 0.0, -1.2], [0.0, 0.2, -1.1]])       # behind the cameras
    add([[0.0, 0.0, -0.5], [0.1, 0.1, 2.8], [-0.1, 0.1, 2.9]])        # crosses the camera plane: dropped
    add([[0.8, 0.1, 2.6], [3.0, 0.2, 2.7], [0.9, 0.4, 2.8]])          # partly off-screen (right)
    add([[-0.2, -2.5, 2.9], [0.1, -0.3, 2.6], [-0.3, -0.2, 2.7]])     # partly off-screen (top)
    add([[5.0, 5.0, 3.0], [6.0, 5.0, 3.0], [5.0, 6.0, 3.0]])          # off-screen altogether
    F.append([0, 1, len(V) + 5])                                      # a vertex index past the end: draws nothing
    tie0 = len(V)
    add([[(20 - 32) / 32.0, (10 - 16) / 32.0, 2.0], [(32 - 32) / 32.0, (10 - 16) / 32.0, 2.0], [(26 - 32) / 32.0, (22 - 16) / 32.0, 2.0]])
    return np.array(V), np.array(F, dtype=np.int32), tie0


def test_vertex_ids_match_the_restatement():
    verts, faces, tie0 = _soup()
    for zn, zf in ((1.0, 3.5), (2.55, 2.9)):
        vid, image = mesh.render_vertex_ids(verts, faces, SK, SOUP_VIEWS, SH, SW, zn, zf)
        rvid, rimage = PN.vertex_ids(verts, faces, SK, SOUP_VIEWS, SH, SW, zn, zf)
        vid, image = vid.cpu().numpy(), image.cpu().numpy()
        assert vid.dtype == np.int32 and image.dtype == np.uint8 and vid.shape == (3, SH, SW)
        assert np.array_equal(vid, rvid), np.argwhere(vid != rvid)[:8]
        assert np.array_equal(image, rimage), np.argwhere(image != rimage)[:8]
        depth, _, face = mesh.render(verts, faces, None, SK, SOUP_VIEWS, SH, SW)
        z = -depth.cpu().numpy().astype(np.float64)
        hit = face.cpu().numpy() >= 0
        assert np.array_equal(vid >= 0, hit & (z >= zn) & (z <= zf))
        for v in range(3):
            assert len(np.unique(vid[v])) > 20
        if zn == 1.0:
            for (x, y), corner in TIE_PIXELS.items():                 # the tie triangle is the nearest surface of view 0
                assert vid[0, y, x] == tie0 + corner, (x, y)
            assert len(np.unique(image)) > 30
        else:
            assert (hit & (z > zf)).any() and (hit & (z < zn)).any() and (vid >= 0).any()
            assert (image[hit & ((z > zf) | (z < zn))] == 0).all()


def test_vertex_ids_without_an_image_and_with_device_inputs():
    verts, faces, _ = _soup()
    vid, image = mesh.render_vertex_ids(verts, faces, SK, SOUP_VIEWS, SH, SW, 1.0, 3.5)
    lib = _lib.load()
    dev, V, F, msh, views, ws = mesh._render_args(torch.from_numpy(verts).cuda(), torch.from_numpy(faces).cuda(), SK, SOUP_VIEWS, SH, SW, 1.0,
                                                  0.0, 0.0, 1e-3, None)
    out = torch.full((3 * SH * SW + 8,), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.dfh_render_raster(*msh, *views, current_stream_ptr()), "dfh_render_raster")
    _lib.check(lib.dfh_render_vertex_ids(*msh, *views, 1.0, 3.5, out.data_ptr(), 0, current_stream_ptr()), "dfh_render_vertex_ids")
    assert torch.equal(out[:3 * SH * SW].view(3, SH, SW), vid) and (out[3 * SH * SW:] == -7).all()


def test_24_views_equal_24_single_view_calls():
    verts, faces, _ = _soup()
    K, lws = descriptors.turntable_views(width=SW, height=SH, dis=260)
    P = verts - np.array([0.0, 0.0, 2.6])                             # the soup around the turntable's axis
    vid, image = mesh.render_vertex_ids(P, faces, K, lws, SH, SW, 1.0, 3.5)
    assert vid.shape == (24, SH, SW) and image.shape == (24, SH, SW)
    covered = (vid >= 0).sum(dim=(1, 2)).cpu().numpy()
    assert (covered > 50).all(), covered
    for v in range(24):
        v1, i1 = mesh.render_vertex_ids(P, faces, K, lws[v], SH, SW, 1.0, 3.5)
        assert torch.equal(v1[0], vid[v]) and torch.equal(i1[0], image[v]), v
    assert not torch.equal(vid[0], vid[16])                           # the second batch is its own views, not the first's again


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
R3, SIZE, ZN, ZF = 32, 128, 1.0, 3.5


def _sphere_volume():
    g = np.arange(R3, dtype=np.float64)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    d = np.sqrt((X - 15.3) ** 2 + (Y - 15.8) ** 2 + (Z - 15.6) ** 2) - 11.2
    return np.clip(d, -3.0, 3.0).astype(np.float32)


class BackProject:
    """feature_fn: every pixel's grey level back to a point of the regularised model, three channels."""

    def __init__(self, K, lws):
        self.K = torch.from_numpy(K).cuda()
        lw = torch.from_numpy(lws).cuda()
        self.Ainv, self.t = torch.linalg.inv(lw[:, :, :3]), lw[:, :, 3]
        self.calls = 0

    def __call__(self, image):
        self.calls += 1
        assert image.dtype == torch.uint8 and image.is_cuda and image.shape == (len(self.t), SIZE, SIZE)
        ys, xs = torch.meshgrid(torch.arange(SIZE, device="cuda", dtype=torch.float64), torch.arange(SIZE, device="cuda", dtype=torch.float64),
                                indexing="ij")
        d = ZF - (image.to(torch.float64) + 0.5) / 255.0 * (ZF - ZN)  # the middle of the grey level's depth interval
        c = torch.stack([(xs - self.K[0, 2]) * d / self.K[0, 0], (ys - self.K[1, 2]) * d / self.K[1, 1], d], dim=-1)
        X = torch.einsum("vij,vhwj->vhwi", self.Ainv, c - self.t[:, None, None, :])
        return X.to(torch.float32)


def _longest_adjacent_edge(verts, faces):
    out = np.zeros(len(verts))
    for a, b in ((0, 1), (1, 2), (2, 0)):
        e = np.linalg.norm(verts[faces[:, a]] - verts[faces[:, b]], axis=1)
        np.maximum.at(out, faces[:, a], e)
        np.maximum.at(out, faces[:, b], e)
    return out


def _bound(reg, faces):
    """Per vertex: its longest adjacent edge + one grey level of depth + one pixel's footprint at zfar."""
    footprint = ZF * 2.0 * np.tan(np.radians(35.0)) / SIZE
    return _longest_adjacent_edge(reg, faces) + (ZF - ZN) / 255.0 + footprint


def test_end_to_end_descriptors_are_positions():
    vol = _sphere_volume()
    verts, faces = (x for x in mesh.marching_cubes(torch.from_numpy(vol).cuda(), as_numpy=True)[:2])
    verts = verts.astype(np.float64)
    K, lws = descriptors.turntable_views(width=SIZE, height=SIZE)
    fn = BackProject(K, lws)
    pd = descriptors.PooledDescriptors(fn, width=SIZE, height=SIZE)
    D = pd(verts, faces)
    assert fn.calls == 1 and D.shape == (len(verts), 3) and D.dtype == np.float32
    reg = descriptors.regularize_mesh(verts)
    cnt = pd.last_count.cpu().numpy()
    seen = cnt > 0
    err = np.linalg.norm(D.astype(np.float64) - reg, axis=1)
    bound = _bound(reg, faces)
    print("vertices %d, seen %.4f, worst error / bound %.3f, median %.3f" % (len(verts), seen.mean(), (err / bound)[seen].max(),
                                                                               np.median((err / bound)[seen])))
    assert (err[seen] <= bound[seen]).all()
    # Seen by some view: 89.45 % on the numpy restatement of this very scene (2350 vertices), not the 95 % first hoped for.  The
    # cameras stand on a horizontal ring of radius 2 around a sphere of radius 0.9: a point with outward normal n is visible iff
    # 2 cos(angle between n and the camera's direction) > 0.9, so the two caps above 63.3 degrees of latitude, 1 - sin(63.3 deg)
    # = 10.7 % of the area, face no camera.
    assert seen.mean() >= 0.89
    # a feature function whose result does not fit the images is refused
    with pytest.raises(ValueError, match="feature_fn"):
        descriptors.PooledDescriptors(lambda im: torch.zeros((24, SIZE, SIZE + 1, 3), device="cuda"), width=SIZE, height=SIZE)(verts, faces)

    # the CNN branch of Fusion with the hook, the default tolerance: every kept vertex's correspondence is near the vertex itself.
    # A vertex no view shows has the descriptor 0 and takes the first live vertex with that descriptor, wherever it is; the
    # point-to-plane pruning removes those that land far away.  Kept: 91.2 % on the numpy restatement (the share seen, below).
    fu = Fusion(vol, 3.0, subsample_rate=3.0, knn=4, marching_cubes_step_size=2, write_warpfield=False)
    fu._lw = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
    fu.initialize_canonical()
    fu._nodes = [(nd[0], nd[1], np.array([1.0, 0, 0, 0, 0, 0, 0, 0]), nd[3]) for nd in fu._nodes]   # an undeformed graph
    cverts, cfaces = np.asarray(fu._vertices, dtype=np.float64), np.asarray(fu._faces)
    cbound = _bound(descriptors.regularize_mesh(cverts), cfaces)
    scale = 1.8 / (cverts[:, 1].max() - cverts[:, 1].min())           # voxels -> regularised units
    fu.descriptor_fn = descriptors.PooledDescriptors(BackProject(K, lws), width=SIZE, height=SIZE)
    fu.setupCorrespondences(vol, method='cnn', prune_result=True)
    assert fu.descriptor_fn.feature_fn.calls == 2 and len(fu.descriptor_fn.last_count) == len(verts)   # (the live mesh came second)
    kept = np.asarray(fu._vertices, dtype=np.float64)
    Ck = np.asarray(fu._correspondences)
    index = {tuple(p): i for i, p in enumerate(cverts)}
    kb = np.array([cbound[index[tuple(p)]] for p in kept])
    dk = np.linalg.norm(Ck - kept, axis=1) * scale
    print("kept %d of %d canonical vertices, worst distance / (2 bound) %.3f" % (len(kept), len(cverts), (dk / (2 * kb)).max()))
    assert (dk <= 2 * kb).all()
    assert 0.85 * len(cverts) <= len(kept) <= len(cverts)
