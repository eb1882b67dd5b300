"""CPU: the depth preprocessing entry point's argument checks (before any launch: device pointers are dummy integers nothing
dereferences), its tables, and the numpy restatement on the fixtures the GPU tests compare the kernel against -- so that those
cannot pass on empty classes -- and on a noisy scene: the filter the header specifies does filter."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import depth_prep_cases as C
import depth_prep_np as DN
from dynamicfusion_body_amd import _lib, build, kernels, scene
from dynamicfusion_body_amd.depth_prep import DepthPrep

BADARG = -1
PTR, PTR2, PTR3 = 0x1000, 0x2000, 0x3000                   # "device pointers"
EYE = (1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0)


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def on_own_thread(test):
    """dfh_last_error() is kept per thread: refused calls are made on a thread of their own (as tests/test_abi_badargs.py does)."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        with ThreadPoolExecutor(1) as ex:
            return ex.submit(test, *args, **kwargs).result()
    return run


def _params(**over):
    f = dict(n_views=1, depth=[PTR], depth_dtype=_lib.F32, H=8, W=8, radius=1, spatial=PTR2, range_lut=PTR2, n_lut=16,
             range_scale=1.0, max_jump=0.1, min_cos=0.5, mask=1)
    f.update(over)
    ptrs = None if f["depth"] is None else (ctypes.c_void_p * max(1, len(f["depth"])))(*f["depth"])
    p = _lib.DepthPrepParams(f["n_views"], ptrs, f["depth_dtype"], f["H"], f["W"], (ctypes.c_double * 9)(*EYE), f["radius"],
                             f["spatial"], f["range_lut"], f["n_lut"], f["range_scale"], f["max_jump"], f["min_cos"], f["mask"])
    p.keep = ptrs
    return p


# one case per rule of dfh_depth_prep_params (include/dfusion_hip.h): name -> (struct overrides, clean, normals)
BAD = {
    "no views": (dict(n_views=0), PTR3, PTR3),
    "17 views": (dict(n_views=17, depth=[PTR] * 17), PTR3, PTR3),
    "null depth array": (dict(depth=None), PTR3, PTR3),
    "null depth entry": (dict(n_views=2, depth=[PTR, None]), PTR3, PTR3),
    "bad dtype": (dict(depth_dtype=2), PTR3, PTR3),
    "H < 2": (dict(H=1), PTR3, PTR3),
    "W < 2": (dict(W=1), PTR3, PTR3),
    "H * W >= 2^31": (dict(H=65536, W=32768), PTR3, PTR3),
    "radius < 0": (dict(radius=-1), PTR3, PTR3),
    "radius > 8": (dict(radius=9), PTR3, PTR3),
    "null spatial": (dict(spatial=None), PTR3, PTR3),
    "null range_lut": (dict(range_lut=None), PTR3, PTR3),
    "n_lut 0": (dict(n_lut=0), PTR3, PTR3),
    "n_lut 4097": (dict(n_lut=4097), PTR3, PTR3),
    "n_lut 0 at radius 0": (dict(n_lut=0, radius=0), PTR3, PTR3),
    "range_scale 0": (dict(range_scale=0.0), PTR3, PTR3),
    "range_scale < 0": (dict(range_scale=-1.0), PTR3, PTR3),
    "range_scale nan": (dict(range_scale=float("nan")), PTR3, PTR3),
    "range_scale inf": (dict(range_scale=float("inf")), PTR3, PTR3),
    "max_jump < 0": (dict(max_jump=-1e-3), PTR3, PTR3),
    "max_jump nan": (dict(max_jump=float("nan")), PTR3, PTR3),
    "max_jump inf": (dict(max_jump=float("inf")), PTR3, PTR3),
    "min_cos < 0": (dict(min_cos=-0.1), PTR3, PTR3),
    "min_cos > 1": (dict(min_cos=1.5), PTR3, PTR3),
    "min_cos nan": (dict(min_cos=float("nan")), PTR3, PTR3),
    "mask 2": (dict(mask=2), PTR3, PTR3),
    "mask -1": (dict(mask=-1), PTR3, PTR3),
    "both outputs null": (dict(), None, None),
    "clean is an input": (dict(n_views=2, depth=[PTR, PTR3]), PTR3, None),
    "normals is an input": (dict(), PTR3, PTR),
}


@pytest.mark.parametrize("name", sorted(BAD))
@on_own_thread
def test_depth_prep_refuses_bad_arguments(lib, name):
    over, clean, normals = BAD[name]
    rc = lib.dfh_depth_prep(_params(**over), clean, normals, None)
    assert rc == BADARG, (name, rc)
    assert b"dfh_depth_prep" in lib.dfh_last_error(), lib.dfh_last_error()


@on_own_thread
def test_depth_prep_refuses_null_params(lib):
    assert lib.dfh_depth_prep(None, PTR3, PTR3, None) == BADARG
    assert b"dfh_depth_prep" in lib.dfh_last_error()
    assert lib.dfh_depth_prep_tile(None) == BADARG
    assert b"dfh_depth_prep_tile" in lib.dfh_last_error()


def test_tile_query(lib):
    th, tw = kernels.depth_prep_tile()
    assert th > 0 and tw > 0


def test_wrapper_checks_need_no_device():
    """What kernels.depth_prep can refuse without a device, it refuses before it asks for one."""
    import torch
    tab = kernels.depth_prep_tables(1, 1.5, 0.05, device="cpu")
    d = torch.zeros(4, 5)
    with pytest.raises(ValueError):
        kernels.depth_prep([], np.eye(3), tab, 0.1, 0.5)
    with pytest.raises(ValueError):
        kernels.depth_prep([d] * 17, np.eye(3), tab, 0.1, 0.5)
    with pytest.raises(ValueError):
        kernels.depth_prep([d, torch.zeros(4, 6)], np.eye(3), tab, 0.1, 0.5)
    with pytest.raises(ValueError):
        kernels.depth_prep([d, d.double()], np.eye(3), tab, 0.1, 0.5)
    with pytest.raises(ValueError):
        kernels.depth_prep_tables(9, 1.5, 0.05, device="cpu")
    with pytest.raises(ValueError):
        kernels.depth_prep_tables(1, 1.5, 0.05, n_lut=4097, device="cpu")
    with pytest.raises(ValueError):
        DepthPrep(min_cos=1.5)


@pytest.mark.parametrize("radius,sigma_s,sigma_r,n_lut,cut", [(0, 1.0, 0.01, 1, 3.0), (3, 1.5, 0.01, 1024, 3.0), (8, 4.0, 0.2, 4096, 2.5)])
def test_tables_follow_the_formulas(radius, sigma_s, sigma_r, n_lut, cut):
    sp, lut, s = kernels.depth_prep_tables(radius, sigma_s, sigma_r, n_lut=n_lut, cut=cut, device="cpu")
    assert sp.dtype.is_floating_point and sp.numpy().dtype == np.float32 and lut.numpy().dtype == np.float32
    assert tuple(sp.shape) == (2 * radius + 1, 2 * radius + 1) and tuple(lut.shape) == (n_lut,)
    assert isinstance(s, float) and s == float(np.float32(n_lut / (cut * sigma_r) ** 2))
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            assert sp[dy + radius, dx + radius].item() == float(np.float32(np.exp(-(dx * dx + dy * dy) / (2 * sigma_s ** 2))))
    want = np.exp(-((np.arange(n_lut) + 0.5) / s) / (2 * sigma_r ** 2)).astype(np.float32)
    assert np.array_equal(lut.numpy(), want)
    assert sp[radius, radius].item() == 1.0 and (np.diff(lut.numpy()) <= 0).all()


# ---- the fixtures, on the restatement alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("size", C.SCENE_SIZES)
def test_scene_fixture_fills_every_class(size):
    """Pixels with a normal, pixels dropped for a missing neighbour or a depth jump, pixels dropped as grazing: >= 10 each (a
    prototype of the restatement counted 838 / 470 / 609 at 37 x 53 and 672 / 344 / 280 at 19 x 70).  The planted bad values
    come out finite, and 0 where the input was not a measurement."""
    H, W = size
    d = C.scene_map(H, W)
    sp, lut, s = C.tables_np(2)
    cls = []
    clean, nrm = DN.depth_prep([d], C.scene_kinv(), 2, sp, lut, s, C.SCENE_JUMP, C.SCENE_COS, mask=False, classes=cls)
    cls = cls[0]
    counts = {k: int(v.sum()) for k, v in cls.items()}
    print(size, counts)
    assert counts["has"] >= 10 and counts["neighbour"] >= 10 and counts["grazing"] >= 10, counts
    assert np.isfinite(clean).all() and np.isfinite(nrm).all()
    bad = ~DN.valid(d)
    assert bad.sum() >= len(C.BAD_VALUES) - 1 + 10
    assert (clean[0][bad] == 0).all() and (nrm[0][bad] == 0).all()
    planted = [(H // 2 - 3 + i, W // 2 - 3 + i) for i in range(len(C.BAD_VALUES))]
    assert [bool(bad[p]) for p in planted] == [True] * 5 + [False]           # -2^-140 is a measurement
    assert clean[0][planted[-1]] < 0
    # unit normals where there is one, facing the camera (the viewing ray is rho = Kinv [x, y, 1], z > 0)
    ln = np.linalg.norm(nrm[0].astype(np.float64), axis=-1)
    assert np.abs(ln[cls["has"]] - 1).max() < 1e-6 and (ln[~cls["has"]] == 0).all()
    masked = DN.depth_prep([d], C.scene_kinv(), 2, sp, lut, s, C.SCENE_JUMP, C.SCENE_COS, mask=True)[0]
    assert np.array_equal(masked[0] != 0, cls["has"]) and np.array_equal(masked[0][cls["has"]], clean[0][cls["has"]])
    for edge in (masked[0][0], masked[0][-1], masked[0][:, 0], masked[0][:, -1]):
        assert (edge == 0).all()


def test_float64_fixture_rounds_at_load():
    d = C.scene_map(37, 53, dtype="float64")
    assert not np.array_equal(d.astype(np.float32).astype(np.float64), d)
    assert d[1, 2] < 0 and d.astype(np.float32)[1, 2] == 0 and np.signbit(d.astype(np.float32)[1, 2])
    sp, lut, s = C.tables_np(1)
    a = DN.depth_prep([d], C.scene_kinv(), 1, sp, lut, s, C.SCENE_JUMP, C.SCENE_COS, mask=False)
    b = DN.depth_prep([d.astype(np.float32)], C.scene_kinv(), 1, sp, lut, s, C.SCENE_JUMP, C.SCENE_COS, mask=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0][0][1, 2] == 0


def test_exact_tie_fixture_has_its_ties():
    d, k = C.tie_map()
    dk = np.abs(np.diff(k, axis=1))
    n_jump = int((dk == 4).sum())                                              # |delta| == max_jump exactly
    n_lut_tie = int((dk == 16).sum())                                          # q == n_lut exactly: excluded
    print("tie fixture: %d pairs at the jump, %d at the table's end" % (n_jump, n_lut_tie))
    assert n_jump >= 10 and n_lut_tie >= 10
    delta = np.diff(d, axis=1)
    assert np.array_equal(np.abs(delta)[dk == 4], np.full(n_jump, np.float32(C.TIE_JUMP)))
    q = (delta * delta) * np.float32(C.TIE_SCALE)
    assert q.dtype == np.float32 and np.array_equal(q, (dk * dk).astype(np.float32))         # integer LUT boundaries, exact
    assert np.array_equal(q[dk == 16], np.full(n_lut_tie, np.float32(C.TIE_NLUT)))
    # the jump tie decides normals at radius 0 (F = d): a pair at exactly max_jump passes, one quantum beyond does not.  With k
    # uniform in 0..63 four neighbours within the jump are rare, so the dense variant of the fixture carries this class
    sp, lut, s = C.tie_tables(0)
    for (dd, kk), least in ((C.tie_map(), 0), (C.tie_map_dense(), 10)):
        cls = []
        DN.depth_prep([dd], np.eye(3), 0, sp, lut, s, C.TIE_JUMP, 0.0, classes=cls)
        ok = ~cls[0]["neighbour"][1:-1, 1:-1]
        adk = np.abs(kk[1:-1, 1:-1, None] - np.stack([kk[1:-1, :-2], kk[1:-1, 2:], kk[:-2, 1:-1], kk[2:, 1:-1]], axis=-1))
        assert np.array_equal(ok, (adk <= 4).all(-1))
        assert int((ok & (adk == 4).any(-1)).sum()) >= least                   # kept although a neighbour sits AT the jump
        assert int((~ok & (adk.max(-1) == 5)).sum()) >= least                  # dropped one quantum beyond it
    # the table's end decides taps at radius 1: a tap with dk = 16 must not count, one with dk = 15 must
    sp, lut, s = C.tie_tables(1)
    F = DN.bilateral(d, 1, sp, lut, s)
    kp = np.pad(k, 1, constant_values=10 ** 6)
    dp = np.pad(d.astype(np.float64), 1)
    num = np.zeros(d.shape)
    den = np.zeros(d.shape)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            kk = kp[1 + dy:1 + dy + 24, 1 + dx:1 + dx + 40]
            q = (kk - k) ** 2
            w = np.where(q < 256, float(sp[dy + 1, dx + 1]) * lut[np.minimum(q, 255)].astype(np.float64), 0.0)
            num += w * dp[1 + dy:1 + dy + 24, 1 + dx:1 + dx + 40]
            den += w
    assert np.abs(F - num / den).max() < 1e-6                                  # (float64 accumulation of the same taps)


def test_the_specified_filter_filters():
    """C1 at 240 x 320, Gaussian noise of 3 mm, DepthPrep's defaults, all on the restatement.  Over the pixels that have a normal
    in the noise-free map, in the noisy map and in the filtered noisy map: the RMS depth error against the noise-free map and the
    median angle between the normals and the noise-free map's normals.  A prototype measured 3.00 -> 1.45 mm and 12.5 -> 4.75
    degrees, this restatement 3.00 -> 1.37 mm and 12.54 -> 4.75 degrees over 67 259 pixels; asserted: ratios below 0.6 and 0.5."""
    H, W, f, cx, cy = scene.CAMERAS["C1"]
    K = scene.intrinsics(f, cx, cy)
    Kinv = np.linalg.inv(K)
    truth = scene.render_depth(K, scene.view_extrinsic(20.0), H, W, invalid_frac=0.02, dtype=np.float64)
    noise = np.random.default_rng(7).normal(0.0, 0.003, size=truth.shape)
    noisy = np.where(truth < 0, truth + noise, 0.0).astype(np.float32)
    truth = truth.astype(np.float32)
    p = DepthPrep()
    sp, lut, s = (t.numpy() if hasattr(t, "numpy") else t for t in kernels.depth_prep_tables(p.radius, p.sigma_s, p.sigma_r, p.n_lut,
                                                                                            p.cut, device="cpu"))

    def run(d, radius):
        cls = []
        c, n = DN.depth_prep([d], Kinv, radius, sp if radius else None, lut, s, p.max_jump, p.min_cos, mask=False, classes=cls)
        return c[0].astype(np.float64), n[0].astype(np.float64), cls[0]["has"]
    c_t, n_t, h_t = run(truth, 0)
    c_n, n_n, h_n = run(noisy, 0)
    c_f, n_f, h_f = run(noisy, p.radius)
    m = h_t & h_n & h_f
    assert m.sum() > 0.5 * H * W

    def rms(c):
        return float(np.sqrt(np.mean((c[m] - c_t[m]) ** 2)))

    def angle(n):
        return float(np.median(np.degrees(np.arccos(np.clip((n[m] * n_t[m]).sum(-1), -1.0, 1.0)))))
    r0, r1, a0, a1 = rms(c_n), rms(c_f), angle(n_n), angle(n_f)
    print("rms %.3f -> %.3f mm, median normal error %.2f -> %.2f deg over %d pixels" % (r0 * 1e3, r1 * 1e3, a0, a1, int(m.sum())))
    assert r1 / r0 < 0.6, (r0, r1)
    assert a1 / a0 < 0.5, (a0, a1)
