"""CPU: the RGB-D ingest entry point's argument checks (before any launch: device pointers are dummy integers nothing
dereferences), its struct mirrors, the Netpbm readers and writers, and the numpy restatement (tests/ingest_np.py) on what the
stage is for: the identity configuration, the occlusion scene whose counts are recorded in tests/golden/ingest_occlusion.json, a
distorted raw image, and the boundary fixtures the GPU tests compare the kernels on (tests/ingest_cases.py) -- so that those
cannot pass on empty classes.

    python tests/test_ingest.py --write      rewrites the record
"""
import ctypes
import functools
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ingest_cases as C               # noqa: E402
import ingest_np as N                  # noqa: E402
from dynamicfusion_body_amd import _lib, build, io as dio          # noqa: E402
from dynamicfusion_body_amd.ingest import DEFAULT_OCCL_TOL, RGBDCalibration, RGBDIngest           # noqa: E402

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ingest_occlusion.json")
BADARG = -1
PTR, PTR2, PTR3, PTR4 = 0x1000, 0x2000, 0x3000, 0x4000       # "device pointers"
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def on_own_thread(test):
    """dfh_last_error() is kept per thread: refused calls are made on a thread of their own (as tests/test_depth_prep.py does)."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        with ThreadPoolExecutor(1) as ex:
            return ex.submit(test, *args, **kwargs).result()
    return run


def _view(**over):
    f = dict(fd=(100.0, 100.0, 4.0, 4.0), kd=(0.0,) * 5, fc=(100.0, 100.0, 4.0, 4.0), kc=(0.0,) * 5,
             T_dc=(1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0))
    f.update(over)
    return _lib.RGBDView(*[(ctypes.c_double * len(f[k]))(*f[k]) for k in ("fd", "kd", "fc", "kc", "T_dc")])


def _params(**over):
    f = dict(n_views=1, raw_depth=[PTR], raw_color=[PTR2], Hd=8, Wd=8, Hc=8, Wc=8, C=3, fx=100.0, fy=100.0, cx=4.0, cy=4.0,
             depth_scale=1e-3, z_min=0.0, z_max=0.0, occl_tol=0.05, max_splat=8, sample=1, views=[_view()])
    f.update(over)

    def arr(ptrs):
        return None if ptrs is None else (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)
    d, c = arr(f["raw_depth"]), arr(f["raw_color"])
    v = None if f["views"] is None else (_lib.RGBDView * max(1, len(f["views"])))(*f["views"])
    p = _lib.RGBDIngestParams(f["n_views"], d, c, f["Hd"], f["Wd"], f["Hc"], f["Wc"], f["C"], f["fx"], f["fy"], f["cx"], f["cy"],
                              f["depth_scale"], f["z_min"], f["z_max"], f["occl_tol"], f["max_splat"], f["sample"], v)
    p.keep = (d, c, v)
    return p


def _edit(values, at, v):
    values = list(values)
    values[at] = v
    return tuple(values)


EYE12 = (1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0)
# one case per rule of dfh_rgbd_ingest (include/dfusion_hip.h): name -> (struct overrides, depth_out, color_out, zbuf)
BAD = {
    "no views": (dict(n_views=0), PTR3, PTR3, PTR4),
    "17 views": (dict(n_views=17, raw_depth=[PTR] * 17, raw_color=[PTR2] * 17, views=[_view()] * 17), PTR3, PTR3, PTR4),
    "null depth array": (dict(raw_depth=None), PTR3, PTR3, PTR4),
    "null depth entry": (dict(n_views=2, raw_depth=[PTR, None], raw_color=[PTR2] * 2, views=[_view()] * 2), PTR3, PTR3, PTR4),
    "null colour entry": (dict(n_views=2, raw_depth=[PTR] * 2, raw_color=[PTR2, None], views=[_view()] * 2), PTR3, PTR3, PTR4),
    "null views": (dict(views=None), PTR3, PTR3, PTR4),
    "Hd < 2": (dict(Hd=1), PTR3, PTR3, PTR4),
    "Wd < 2": (dict(Wd=1), PTR3, PTR3, PTR4),
    "Hc < 2": (dict(Hc=1), PTR3, PTR3, PTR4),
    "Wc < 2": (dict(Wc=1), PTR3, PTR3, PTR4),
    "Hd * Wd >= 2^31": (dict(Hd=65536, Wd=32768), PTR3, PTR3, PTR4),
    "Hc * Wc >= 2^31": (dict(Hc=65536, Wc=32768), PTR3, PTR3, PTR4),
    "C 2": (dict(C=2), PTR3, PTR3, PTR4),
    "C 5": (dict(C=5), PTR3, PTR3, PTR4),
    "fx 0": (dict(fx=0.0), PTR3, PTR3, PTR4),
    "fy < 0": (dict(fy=-1.0), PTR3, PTR3, PTR4),
    "fx inf": (dict(fx=INF), PTR3, PTR3, PTR4),
    "cx nan": (dict(cx=NAN), PTR3, PTR3, PTR4),
    "depth fx 0": (dict(views=[_view(fd=(0.0, 100.0, 4.0, 4.0))]), PTR3, PTR3, PTR4),
    "depth fy nan": (dict(views=[_view(fd=(100.0, NAN, 4.0, 4.0))]), PTR3, PTR3, PTR4),
    "colour fx < 0": (dict(views=[_view(fc=(-100.0, 100.0, 4.0, 4.0))]), PTR3, PTR3, PTR4),
    "colour fy inf": (dict(views=[_view(fc=(100.0, INF, 4.0, 4.0))]), PTR3, PTR3, PTR4),
    "kd nan": (dict(views=[_view(kd=(0.0, NAN, 0.0, 0.0, 0.0))]), PTR3, PTR3, PTR4),
    "kc inf": (dict(views=[_view(kc=(0.0, 0.0, 0.0, 0.0, INF))]), PTR3, PTR3, PTR4),
    "T_dc nan": (dict(views=[_view(T_dc=_edit(EYE12, 7, NAN))]), PTR3, PTR3, PTR4),
    "second view's cd inf": (dict(n_views=2, raw_depth=[PTR] * 2, raw_color=[PTR2] * 2,
                                  views=[_view(), _view(fd=(100.0, 100.0, 4.0, INF))]), PTR3, PTR3, PTR4),
    "depth_scale 0": (dict(depth_scale=0.0), PTR3, PTR3, PTR4),
    "depth_scale < 0": (dict(depth_scale=-1e-3), PTR3, PTR3, PTR4),
    "depth_scale nan": (dict(depth_scale=NAN), PTR3, PTR3, PTR4),
    "depth_scale inf": (dict(depth_scale=INF), PTR3, PTR3, PTR4),
    "z_min nan": (dict(z_min=NAN), PTR3, PTR3, PTR4),
    "z_max nan": (dict(z_max=NAN), PTR3, PTR3, PTR4),
    "occl_tol < 0": (dict(occl_tol=-1e-9), PTR3, PTR3, PTR4),
    "occl_tol nan": (dict(occl_tol=NAN), PTR3, PTR3, PTR4),
    "max_splat 0": (dict(max_splat=0), PTR3, PTR3, PTR4),
    "max_splat 17": (dict(max_splat=17), PTR3, PTR3, PTR4),
    "sample 2": (dict(sample=2), PTR3, PTR3, PTR4),
    "sample -1": (dict(sample=-1), PTR3, PTR3, PTR4),
    "null depth_out": (dict(), None, PTR3, PTR4),
    "colour without color_out": (dict(), PTR3, None, PTR4),
    "colour without zbuf": (dict(), PTR3, PTR3, None),
    "zbuf not 8-byte aligned": (dict(), PTR3, PTR3, PTR4 + 4),
    "4-channel image not 4-byte aligned": (dict(C=4, raw_color=[PTR2 + 2]), PTR3, PTR3, PTR4),
}


@pytest.mark.parametrize("name", sorted(BAD))
@on_own_thread
def test_rgbd_ingest_refuses_bad_arguments(lib, name):
    over, depth_out, color_out, zbuf = BAD[name]
    rc = lib.dfh_rgbd_ingest(_params(**over), depth_out, color_out, PTR3, zbuf, None)
    assert rc == BADARG, (name, rc)
    assert b"dfh_rgbd_ingest" in lib.dfh_last_error(), lib.dfh_last_error()


@on_own_thread
def test_rgbd_ingest_refuses_null_params(lib):
    assert lib.dfh_rgbd_ingest(None, PTR3, PTR3, PTR3, PTR4, None) == BADARG
    assert b"dfh_rgbd_ingest" in lib.dfh_last_error()
    assert lib.dfh_rgbd_ingest_tile(None) == BADARG
    assert b"dfh_rgbd_ingest_tile" in lib.dfh_last_error()


def test_tile_and_workspace_queries(lib):
    hw = (ctypes.c_int * 2)()
    assert lib.dfh_rgbd_ingest_tile(hw) == 0 and hw[0] > 0 and hw[1] > 0
    assert lib.dfh_rgbd_ingest_workspace_bytes(3, 7, 9) >= 4 * 3 * 7 * 9
    assert lib.dfh_rgbd_ingest_workspace_bytes(3, 7, 9) % 8 == 0
    for bad in ((0, 8, 8), (17, 8, 8), (1, 1, 8), (1, 8, 1), (1, 65536, 32768)):
        assert lib.dfh_rgbd_ingest_workspace_bytes(*bad) == 0


def test_struct_mirrors_are_listed():
    """tests/test_abi_symbols.py compares every struct of _lib.STRUCTS with the C compiler's layout: the new ones are among them."""
    assert _lib.STRUCTS["dfh_rgbd_view"] is _lib.RGBDView and _lib.STRUCTS["dfh_rgbd_ingest_params"] is _lib.RGBDIngestParams
    assert ctypes.sizeof(_lib.RGBDView) == 30 * 8
    assert _lib.ABI_VERSION == 8


def test_python_objects_check_without_a_device():
    cal = RGBDCalibration((100.0, 100.0, 4.0, 4.0))
    assert cal.record().shape == (30,) and np.array_equal(cal.record()[18:], np.eye(4)[:3].reshape(-1))
    ing = RGBDIngest([cal], (8, 8), (8, 8), (100.0, 50.0, 4.0, 3.0))
    assert np.array_equal(ing.K, [[100.0, 0, 4.0], [0, 50.0, 3.0], [0, 0, 1.0]]) and np.allclose(ing.Kinv @ ing.K, np.eye(3))
    assert ing.occl_tol == DEFAULT_OCCL_TOL
    for bad in (dict(max_splat=0), dict(max_splat=17), dict(sample="cubic"), dict(occl_tol=-1.0), dict(depth_scale=0.0)):
        with pytest.raises(ValueError):
            RGBDIngest([cal], (8, 8), (8, 8), (100.0, 100.0, 4.0, 4.0), **bad)
    with pytest.raises(ValueError):
        RGBDIngest([], (8, 8), (8, 8), (100.0, 100.0, 4.0, 4.0))
    with pytest.raises(ValueError):
        RGBDCalibration((100.0, 0.0, 4.0, 4.0))
    with pytest.raises(ValueError):
        RGBDCalibration((100.0, 100.0, 4.0, 4.0), depth_distortion=(NAN, 0, 0, 0, 0))
    with pytest.raises(ValueError):
        ing([np.zeros((8, 8), np.uint16)] * 2)                     # two maps for one calibrated view: refused before any device


# ---- Netpbm -------------------------------------------------------------------------------------------------------------------
def test_pgm16_round_trip(tmp_path):
    a = np.random.default_rng(3).integers(0, 65536, size=(5, 7)).astype(np.uint16)
    a[0, 0], a[0, 1], a[0, 2] = 0x1234, 0xff00, 0x00ff              # high bytes: the file is big-endian
    path = str(tmp_path / "d.pgm")
    dio.write_pgm16(path, a)
    buf = open(path, "rb").read()
    assert buf.startswith(b"P5\n7 5\n65535\n") and buf[-70:-64] == b"\x12\x34\xff\x00\x00\xff"
    b = dio.read_pgm16(path)
    assert b.dtype == np.uint16 and np.array_equal(a, b)
    with open(path, "wb") as f:                                     # a header with a comment and other whitespace
        f.write(b"P5 # a comment\n 7\t5 # another\n65535\n" + a.astype(">u2").tobytes())
    assert np.array_equal(dio.read_pgm16(path), a)
    with open(path, "wb") as f:
        f.write(b"P5\n7 5\n255\n" + bytes(35))
    with pytest.raises(ValueError):
        dio.read_pgm16(path)                                        # an 8-bit PGM is not a raw depth map
    with open(path, "wb") as f:
        f.write(b"P5\n7 5\n65535\n" + bytes(69))
    with pytest.raises(ValueError):
        dio.read_pgm16(path)                                        # truncated
    with pytest.raises(ValueError):
        dio.write_pgm16(path, a.astype(np.int32))


def test_ppm_round_trip(tmp_path):
    a = np.random.default_rng(4).integers(0, 256, size=(4, 6, 3)).astype(np.uint8)
    path = str(tmp_path / "c.ppm")
    dio.write_ppm(path, a)
    assert open(path, "rb").read().startswith(b"P6\n6 4\n255\n")
    b = dio.read_ppm(path)
    assert b.dtype == np.uint8 and np.array_equal(a, b) and b.flags.writeable
    with pytest.raises(ValueError):
        dio.read_pgm16(path)
    with pytest.raises(ValueError):
        dio.write_ppm(path, a[..., :2])


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_identity_on_the_restatement():
    """Zero distortion, output intrinsics = the raw ones, T_dc the identity, colour the size of depth: depth_out = -raw * scale
    exactly; color_out = the raw colour with X = 255 on every valid pixel left of the last column and above the last row.
    A pixel's splat is the rectangle rint(i - 0.5) .. rint(i + 0.5), which reaches its neighbours, so "every valid pixel" holds
    where no neighbour lies more than occl_tol in front: random depths with the test off (+inf), and depths within 4 cm of each
    other at the shipped tolerance of 5 cm.  depth_scale is 2^-10 and the intrinsics are powers of two, so that x*z is exact and
    (x*z)/z gives x back: u = i and v = j exactly, and the border columns and rows fall where the rule says (with a decimal scale
    the last bit of (x*z)/z decides on which side of 0 and Wc - 1 a border pixel lands)."""
    rng = np.random.default_rng(5)
    H, W = 13, 17
    img = rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    k = (64.0, 64.0, 8.0, 6.0)
    for sample in (0, 1):
        for occl_tol, spread in ((np.inf, 3700), (DEFAULT_OCCL_TOL, 40)):
            raw = rng.integers(300, 300 + spread, size=(H, W)).astype(np.uint16)
            raw[rng.random((H, W)) < 0.1] = 0
            depth, color, cdepth, zbuf = N.ingest(raw[None], img[None], [N.view(k, fc=k)], k, depth_scale=2.0 ** -10, occl_tol=occl_tol,
                                                  sample=sample, max_splat=8)
            assert np.array_equal(depth[0], (-(raw.astype(np.float64) * 2.0 ** -10)).astype(np.float32))
            valid = raw != 0
            assert np.array_equal(depth[0] != 0, valid)
            has = valid.copy()
            has[-1, :] = False
            has[:, -1] = False
            assert np.array_equal(color[0][..., 3] == 255, has) and has.sum() > 100
            assert np.array_equal(color[0][has][:, :3], img[has])
            assert (color[0][~has] == 0).all()
            assert np.array_equal(cdepth[0], np.where(has, depth[0], np.float32(0)))
            # the z-buffer never holds more than a valid pixel's own key at its own place
            key = (raw.astype(np.float64) * 2.0 ** -10).astype(np.float32).view(np.uint32)
            assert (zbuf[0][valid] <= key[valid]).all() and (zbuf[0] != N.EMPTY).sum() >= valid.sum()
    d_only = N.ingest(raw[None], None, [N.view(k)], k, depth_scale=2.0 ** -10)
    assert d_only[1] is None and np.array_equal(d_only[0], depth)


def occlusion_record():
    w_off, has_off, ok_off = N.occlusion_counts(np.inf)
    w_on, has_on, ok_on = N.occlusion_counts(DEFAULT_OCCL_TOL)
    sweep = {}
    for tol in (0.0, 0.01, 0.02, 0.03, 0.05, 0.075, 0.1, 0.2):
        w, _, ok = N.occlusion_counts(tol)
        sweep["%g" % tol] = {"wall_pixels_with_sphere_colour": w, "correct_pixels_dropped": int((ok_off & ~ok).sum())}
    return {"occl_tol_default": DEFAULT_OCCL_TOL,
            "no_test": {"wall_pixels_with_sphere_colour": w_off, "pixels_with_colour": has_off, "correct_pixels": int(ok_off.sum())},
            "default": {"wall_pixels_with_sphere_colour": w_on, "pixels_with_colour": has_on,
                        "correct_pixels_dropped": int((ok_off & ~ok_on).sum())},
            "sweep": sweep}


@pytest.fixture(scope="module")
def record():
    return occlusion_record()


def test_occlusion_scene(record):
    """A sphere (radius 0.5 at z 2) in front of a wall (z 3); 160 x 120 depth at f 150, 320 x 240 colour at f 300, baseline 0.05.
    Measured on this restatement: 102 wall pixels take the sphere's colour without the test, 0 with the shipped default
    occl_tol = 0.05, which drops 108 of 18 692 correctly coloured pixels (0.58 %)."""
    off, on = record["no_test"], record["default"]
    print(json.dumps(record, indent=1))
    assert off["wall_pixels_with_sphere_colour"] >= 50, off                  # the scene does exercise occlusion
    assert on["wall_pixels_with_sphere_colour"] <= off["wall_pixels_with_sphere_colour"] / 10.0, (off, on)
    assert on["correct_pixels_dropped"] < 0.02 * off["correct_pixels"], (off, on)


def test_occlusion_scene_matches_its_record(record):
    with open(RECORD) as f:
        gold = json.load(f)
    assert gold == record
    assert gold["occl_tol_default"] == DEFAULT_OCCL_TOL


def test_distorted_raw_image_comes_back():
    """kd = (0.1, -0.05, 1e-3, -1e-3, 0.01): a raw depth image drawn THROUGH the model (the generator inverts it per raw pixel)
    comes back, on the ideal output pinhole, within one raw pixel of the undistorted ground truth everywhere the source is
    inside: the output value lies within the range the exact scene depth takes over the pixel's +-1 neighbourhood (sampled
    every quarter pixel), up to the raw map's quantisation of half a device unit."""
    kd = (0.1, -0.05, 1e-3, -1e-3, 0.01)
    Hd, Wd = 96, 128
    fd = (110.0, 112.0, 63.5, 47.5)
    out_k = (104.0, 104.0, 63.5, 47.5)
    scale = 1e-3
    sphere = ((0.8, 0.5, 2.0), 0.5)                                  # off the axis, where the model moves a pixel by 2 to 3 pixels
    raw, _, _, _, _ = N.raw_frame((Hd, Wd), fd, kd, (8, 8), fd, (0,) * 5, 0.05, depth_scale=scale, sphere=sphere)
    depth, _, _, _ = N.ingest(raw[None], None, [N.view(fd, kd)], out_k, depth_scale=scale)
    z = -depth[0].astype(np.float64)
    j, i = np.meshgrid(np.arange(Hd, dtype=np.float64), np.arange(Wd, dtype=np.float64), indexing="ij")
    # where the source is inside (the restatement's own test), the output must be valid: the scene has no holes
    x, y = N.ideal(i, j, out_k)
    xd, yd = N.distort(x, y, np.asarray(kd))
    si, sj = np.rint(fd[0] * xd + fd[2]), np.rint(fd[1] * yd + fd[3])
    inside = (si >= 0) & (si <= Wd - 1) & (sj >= 0) & (sj <= Hd - 1)
    assert np.array_equal(z > 0, inside) and inside.mean() > 0.8 and (~inside).sum() > 0
    # one raw pixel is fd/out_k output pixels: +-1.1 output pixels covers it on both axes
    reach = 1.0 * max(out_k[0] / fd[0], out_k[1] / fd[1], 1.0)
    lo = np.full((Hd, Wd), np.inf)
    hi = np.full((Hd, Wd), -np.inf)
    for dy in np.linspace(-reach, reach, 9):
        for dx in np.linspace(-reach, reach, 9):
            gx, gy = N.ideal(i + dx, j + dy, out_k)
            g, _ = N.cast_rays(gx, gy, sphere=sphere)
            lo, hi = np.minimum(lo, g), np.maximum(hi, g)
    tol = 0.5 * scale * (1 + 1e-6) + 2e-7 * 3.0                      # quantisation + the float32 output
    bad = inside & ((z < lo - tol) | (z > hi + tol))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5])
    # and the distortion matters: read without it, the same raw image misses that envelope at many pixels
    plain, _, _, _ = N.ingest(raw[None], None, [N.view(fd)], out_k, depth_scale=scale)
    zp = -plain[0].astype(np.float64)
    assert ((zp > 0) & inside & ((zp < lo - tol) | (zp > hi + tol))).sum() > 50


# ---- the GPU tests' fixtures, on the restatement alone ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.BOUNDARY_CASES))
def test_boundary_fixture_sits_on_its_boundary(name):
    """Every boundary case of tests/ingest_cases.py states what the restatement must give on each side of, and exactly on, its
    boundary; the values involved are exact (power-of-two intrinsics and depths)."""
    case = C.BOUNDARY_CASES[name]()
    out = N.ingest(*case["args"], **case["kw"])
    case["check"](out)


if __name__ == "__main__":
    if "--write" in sys.argv:
        with open(RECORD, "w") as f:
            json.dump(occlusion_record(), f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", RECORD)
