"""CPU: the visible-surface samples' C ABI (dfh_render_samples_*) is declared, exported and bound and refuses arguments it
cannot use before any HIP call, and its numpy restatement (tests/render_samples_np.py, the yardstick of
tests/test_gpu_render_samples.py) gets cases with known answers right.  No kernel is launched: device pointers are dummy
non-null integers that nothing dereferences."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import render_np as RN
import render_samples_np as RS
from dynamicfusion_body_amd import _lib, build
from dynamicfusion_body_amd.pipeline import extract_surface_samples_torch

SYMBOLS = ("dfh_render_samples_workspace_bytes", "dfh_render_samples_count", "dfh_render_samples_emit")
OK, BADARG = 0, -1
PTR = 0x1000
NV, H, W, NF, NVERT = 2, 48, 64, 10, 30
EYE = (ctypes.c_double * 18)(*([1, 0, 0, 0, 1, 0, 0, 0, 1] * 2))
LW = (ctypes.c_double * 24)(*([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] * 2))
CTR = (ctypes.c_double * 3)()


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def test_samples_symbols_declared_exported_bound_at_abi8(lib):
    declared = _lib.declared_symbols()
    raw = ctypes.CDLL(build.LIB)
    for name in SYMBOLS:
        assert name in declared, name
        assert hasattr(raw, name), name
        assert name in _lib._SIGNATURES, name
    assert _lib.ABI_VERSION == 8 and lib.dfh_version() == 8


def test_samples_workspace_size_query(lib):
    """Needs no device.  Bad sizes give 0; the scan's workspace is small beside the keys and shrinks with the stride."""
    n1 = lib.dfh_render_samples_workspace_bytes(3, 480, 640, 1)
    n2 = lib.dfh_render_samples_workspace_bytes(3, 480, 640, 2)
    assert 0 < n2 < n1 < 3 * 480 * 640 * 8 // 100
    for bad in ((0, 480, 640, 1), (17, 480, 640, 1), (1, 0, 640, 1), (1, 480, 0, 1), (1, 480, 640, 0), (1, 480, 640, -2),
                (16, 1 << 17, 1 << 17, 1)):
        assert lib.dfh_render_samples_workspace_bytes(*bad) == 0, bad
    assert lib.dfh_render_samples_workspace_bytes(1, 1, 1, 7) > 0


def _count(lib, nv=NV, h=H, w=W, nf=NF, stride=1, ws=PTR, ws_bytes=None, scan=PTR, scan_bytes=None, total=PTR):
    ws_bytes = lib.dfh_render_workspace_bytes(NV, H, W, NF) if ws_bytes is None else ws_bytes
    scan_bytes = lib.dfh_render_samples_workspace_bytes(NV, H, W, 1) if scan_bytes is None else scan_bytes
    return lib.dfh_render_samples_count(nv, h, w, nf, stride, ws, ws_bytes, scan, scan_bytes, total, None)


def _emit(lib, verts=PTR, cpos=PTR, cnrm=PTR, nvert=NVERT, faces=PTR, nf=NF, nv=NV, K=EYE, lw=LW, h=H, w=W, ctr=CTR, znear=1e-3,
          stride=1, ws=PTR, ws_bytes=None, scan=PTR, scan_bytes=None, pos=PTR, nrm=PTR, pix=PTR, cap=5):
    ws_bytes = lib.dfh_render_workspace_bytes(NV, H, W, NF) if ws_bytes is None else ws_bytes
    scan_bytes = lib.dfh_render_samples_workspace_bytes(NV, H, W, 1) if scan_bytes is None else scan_bytes
    return lib.dfh_render_samples_emit(verts, cpos, cnrm, nvert, faces, nf, nv, K, lw, h, w, 1.0, ctr, 0.0, znear, stride, ws, ws_bytes,
                                       scan, scan_bytes, pos, nrm, pix, cap, None)


def on_own_thread(test):
    """dfh_last_error() is kept per thread: the refused calls are made on a thread of their own (tests/test_abi_badargs.py)."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        with ThreadPoolExecutor(1) as ex:
            return ex.submit(test, *args, **kwargs).result()
    return run


def _refused(lib, name, rc):
    assert rc == BADARG, (name, rc)
    assert name.encode() in lib.dfh_last_error(), (name, lib.dfh_last_error())


@on_own_thread
def test_count_refuses_bad_arguments(lib):
    name = "dfh_render_samples_count"
    for kw in (dict(ws=None), dict(scan=None), dict(total=None),                       # null required pointers
               dict(stride=0), dict(stride=-1),
               dict(nv=0), dict(nv=17), dict(h=0), dict(w=0), dict(nf=-1), dict(nf=1 << 31),
               dict(ws_bytes=lib.dfh_render_workspace_bytes(NV, H, W, NF) - 1), dict(ws_bytes=0),
               dict(scan_bytes=lib.dfh_render_samples_workspace_bytes(NV, H, W, 1) - 1), dict(scan_bytes=0),
               dict(stride=2, scan_bytes=lib.dfh_render_samples_workspace_bytes(NV, H, W, 2) - 1)):
        _refused(lib, name, _count(lib, **kw))


@on_own_thread
def test_emit_refuses_bad_arguments(lib):
    name = "dfh_render_samples_emit"
    for kw in (dict(verts=None), dict(cpos=None), dict(faces=None), dict(K=None), dict(lw=None), dict(ctr=None),
               dict(ws=None), dict(scan=None), dict(pos=None), dict(pix=None),         # null required pointers
               dict(cnrm=None),                                                        # a normal output without canon_nrm
               dict(stride=0), dict(stride=-3),
               dict(nv=0), dict(nv=17), dict(h=0), dict(w=0), dict(nf=-1), dict(nvert=-1), dict(znear=0.0),
               dict(cap=-1),
               dict(ws_bytes=lib.dfh_render_workspace_bytes(NV, H, W, NF) - 1),
               dict(scan_bytes=lib.dfh_render_samples_workspace_bytes(NV, H, W, 1) - 1),
               dict(K=(ctypes.c_double * 18)(*([1, 0, 0, 1, 1, 0, 0, 0, 1] * 2)))):    # K not upper-triangular
        _refused(lib, name, _emit(lib, **kw))
    # nothing to write: no HIP call is made either (capacity 0, or no faces -- nothing can be covered; no normals at all)
    assert _emit(lib, cap=0) == OK and _emit(lib, cap=0, pos=None, nrm=None, pix=None) == OK
    assert _emit(lib, nf=0, verts=None, cpos=None, cnrm=None, faces=None, nrm=None) == OK
    assert _emit(lib, cap=0, cnrm=None, nrm=None) == OK


# ---- the restatement on cases with known answers (cameras of tests/test_render_cpu.py) ---------------------------------------
K64 = np.array([[64.0, 0.0, 0.0], [0.0, 64.0, 0.0], [0.0, 0.0, 1.0]])
LW_ID = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)


def _quad():
    Z = 2.0
    corners = np.array([[8, 4], [40, 4], [40, 36], [8, 36]], dtype=np.float64)
    return np.concatenate([corners * Z / 64.0, np.full((4, 1), Z)], axis=1), np.array([[0, 1, 2], [0, 2, 3]])


def test_fronto_parallel_quad_samples_are_back_projections():
    """canon_pos = verts: a sample is the surface point its pixel sees, here (x, y, 64) * 2 / 64 on the plane z = 2; the
    diagonal's pixels are face 0's, and with the constant normal of the plane every sample's normal is that normal."""
    verts, faces = _quad()
    nrm_in = np.tile(np.array([0.0, 0.0, -3.0]), (4, 1))                 # not unit: the output is normalised
    pos, nrm, pixel = RS.render_samples(verts, faces, verts, nrm_in, K64, LW_ID, 48, 48)
    assert len(pixel) == 33 * 33
    ys, xs = pixel // 48, pixel % 48
    assert ys.min() == 4 and ys.max() == 36 and xs.min() == 8 and xs.max() == 40
    assert np.all(np.diff(pixel) > 0)
    back = np.stack([xs * 2.0 / 64.0, ys * 2.0 / 64.0, np.full(len(xs), 2.0)], axis=1)
    assert np.abs(pos - back).max() <= 1e-12
    assert np.abs(nrm - np.array([0.0, 0.0, -1.0])).max() <= 1e-15
    face = RN.render(verts, faces, None, K64, LW_ID, 48, 48)[2][0]
    on_diag = (xs - 8) == (ys - 4)
    assert np.all(face[ys[on_diag], xs[on_diag]] == 0)
    # the diagonal's samples use face 0's weights: its vertex 1 (the corner off the diagonal's other side) gets weight 0
    only_v1 = np.zeros((4, 3))
    only_v1[1] = 1.0
    p1, _, _ = RS.render_samples(verts, faces, only_v1, None, K64, LW_ID, 48, 48)
    assert np.all(p1[on_diag] == 0.0) and np.all(p1[(xs - 8) > (ys - 4)] > 0.0)


def _tilted():
    K = np.array([[300.5, 0.25, 160.3], [0.0, 301.25, 119.7], [0.0, 0.0, 1.0]])
    a = np.radians(10.0)
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    lw = np.concatenate([R, np.array([[0.05], [-0.02], [0.3]])], axis=1)
    verts = np.array([[-0.6, -0.5, 2.2], [0.7, -0.4, 1.7], [0.1, 0.6, 2.6]])
    return K, lw, verts, np.array([[0, 1, 2]])


def test_tilted_triangle_samples_lie_on_its_plane_and_on_their_pixels():
    K, lw, verts, faces = _tilted()
    pos, nrm, pixel = RS.render_samples(verts, faces, verts, None, K, lw, 240, 320)
    assert nrm is None and len(pixel) > 1000
    n = np.cross(verts[1] - verts[0], verts[2] - verts[0])
    d = n @ verts[0]
    assert np.abs(pos @ n - d).max() <= 1e-12 * np.abs(d)
    u, v, _ = RN.project(pos, K, lw, 1.0, 0.0, 0.0)
    assert np.abs(u - pixel % 320).max() <= 1e-9 and np.abs(v - pixel // 320).max() <= 1e-9


def test_other_attributes_get_the_same_weights():
    """canon_pos != verts: the weights are the pixel's (they sum to 1 and reproduce the surface point), applied to the
    other array -- a linear map of the vertices maps the samples."""
    K, lw, verts, faces = _tilted()
    rng = np.random.default_rng(3)
    M, t = rng.normal(size=(3, 3)), rng.normal(size=3)
    other = verts @ M.T + t
    p0, _, pix0 = RS.render_samples(verts, faces, verts, None, K, lw, 240, 320)
    p1, n1, pix1 = RS.render_samples(verts, faces, other, other, K, lw, 240, 320)
    assert np.array_equal(pix0, pix1)
    assert np.abs(p1 - (p0 @ M.T + t)).max() <= 1e-12 * np.abs(other).max() * 10
    assert np.abs(np.linalg.norm(n1, axis=1) - 1.0).max() <= 1e-15 * 4
    # one-hot attributes read the weights off: each in [0, 1], summing to 1
    b, _, _ = RS.render_samples(verts, faces, np.eye(3), None, K, lw, 240, 320)
    assert b.min() >= 0.0 and b.max() <= 1.0 and np.abs(b.sum(axis=1) - 1.0).max() <= 1e-15 * 4
    # a zero attribute vector gives the zero normal, not a NaN
    _, nz, _ = RS.render_samples(verts, faces, verts, np.zeros((3, 3)), K, lw, 240, 320)
    assert np.all(nz == 0.0)


@pytest.mark.parametrize("stride", [2, 3])
def test_strides_are_subsets_at_the_right_pixels(stride):
    K, lw, verts, faces = _tilted()
    H, W = 239, 317                                                       # neither a multiple of the strides
    p1, n1, pix1 = RS.render_samples(verts, faces, verts, verts, K, lw, H, W)
    ps, ns, pixs = RS.render_samples(verts, faces, verts, verts, K, lw, H, W, stride=stride)
    on = ((pix1 // W) % stride == 0) & ((pix1 % W) % stride == 0)
    assert 0 < len(pixs) < len(pix1)
    assert np.array_equal(pixs, pix1[on]) and np.array_equal(ps, p1[on]) and np.array_equal(ns, n1[on])


@pytest.mark.parametrize("total,cap", [(10, 3), (1000, 999), (1000, 1), (7, 7), (5, 9), (12345, 777), (9, 0)])
def test_capacity_rule_is_the_band_extraction_s(total, cap):
    """subsample_index against the rule as the header states it (first sample of every slot floor(i * cap / total)) and against
    extract_surface_samples_torch on a volume whose band voxels are numbered."""
    keep = RS.subsample_index(total, cap)
    if cap >= total:
        assert np.array_equal(keep, np.arange(total))
    else:
        slot = (np.arange(total, dtype=np.int64) * cap) // total
        first = np.nonzero(np.concatenate([[True], slot[1:] != slot[:-1]]) & (cap > 0))[0]
        assert np.array_equal(keep, first) and len(keep) == cap
        assert np.array_equal(slot[keep], np.arange(cap))
    if 0 < cap and total <= 1000:
        # a z column of `total` band voxels with T rising along z: sample i sits at z = i + 1 (minus a Newton step < 1)
        T = torch.full((3, 3, total + 2), 5.0, dtype=torch.float64)
        T[1, 1, 1:total + 1] = torch.linspace(-0.4, 0.4, total, dtype=torch.float64)
        Wt = torch.zeros_like(T)
        Wt[1, 1, 1:total + 1] = 1.0
        allp, _ = extract_surface_samples_torch(T, Wt, 1.0)
        sub, _ = extract_surface_samples_torch(T, Wt, 1.0, max_samples=cap)
        if len(allp) == total:                                            # (every band voxel has a gradient here)
            assert torch.equal(sub, allp[torch.from_numpy(keep)])


def test_capacity_applies_to_the_restatement():
    K, lw, verts, faces = _tilted()
    p, n, pix = RS.render_samples(verts, faces, verts, verts, K, lw, 120, 160)
    total = len(pix)
    for cap in (0, 1, total - 1, total, total + 5):
        ps, ns, pixs = RS.render_samples(verts, faces, verts, verts, K, lw, 120, 160, max_samples=cap)
        keep = RS.subsample_index(total, cap)
        assert len(pixs) == min(cap, total)
        assert np.array_equal(pixs, pix[keep]) and np.array_equal(ps, p[keep]) and np.array_equal(ns, n[keep])
    if total > 10:
        half = RS.render_samples(verts, faces, verts, verts, K, lw, 120, 160, max_samples=total // 2)[2]
        assert half[-1] > pix[total // 2 + total // 4]                    # an even subsample, not a prefix
