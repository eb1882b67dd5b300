"""Fixtures of the depth preprocessing tests (tests/test_depth_prep.py on the CPU, tests/test_gpu_depth_prep.py on the GPU): the
inputs, the filter tables and, computed once per process and never modified, the numpy restatement's outputs."""
import functools

import numpy as np

from dynamicfusion_body_amd import kernels, scene

SCENE_SIZES = ((37, 53), (19, 70))
SCENE_JUMP, SCENE_COS = 0.12, 0.8
TIE_JUMP, TIE_NLUT, TIE_SCALE = 4.0 / 64.0, 256, 4096.0
# (y, x) -> planted value; the last one is a VALID measurement (finite and negative: a float32 subnormal), the others are not
BAD_VALUES = (np.nan, np.inf, -np.inf, 1.25, -0.0, -2.0 ** -140)


def small_camera():
    """The C1 camera with its intrinsics divided by 6 (a 53 x 40 image would show what C1 shows in 320 x 240)."""
    _, _, f, cx, cy = scene.CAMERAS["C1"]
    return scene.intrinsics(f / 6.0, cx / 6.0, cy / 6.0)


def tables_np(radius, sigma_s=1.5, sigma_r=0.05, n_lut=1024, cut=3.0):
    sp, lut, s = kernels.depth_prep_tables(radius, sigma_s, sigma_r, n_lut, cut, device="cpu")
    return sp.numpy(), lut.numpy(), s


@functools.lru_cache(maxsize=None)
def scene_map(H, W, angle=20.0, seed=1234, dtype="float32", bad=True):
    """render_depth(invalid_frac=0.02) through the small camera, with BAD_VALUES planted on a diagonal inside the sphere."""
    K = small_camera()
    d = scene.render_depth(K, scene.view_extrinsic(angle), H, W, invalid_frac=0.02, seed=seed, dtype=np.float64)
    if dtype == "float64":
        # values that are not float32-exact (the render's own are not; make sure of it), and one that rounds to -0.0
        d = d * (1.0 + 2.0 ** -30)
        d[1, 2] = -1e-50
    d = d.astype(dtype)
    if bad:
        for i, b in enumerate(BAD_VALUES):
            d[H // 2 - 3 + i, W // 2 - 3 + i] = b
    d.setflags(write=False)
    return d


def scene_kinv():
    return np.linalg.inv(small_camera())


@functools.lru_cache(maxsize=None)
def tie_map(seed=5):
    """24 x 40, depths -(1 + k/64), k uniform in 0..63: every difference, its square times 4096 (= dk^2) and every sum below are
    exact in float32, so |delta| == max_jump (dk = 4) and q == n_lut (dk = 16) happen EXACTLY, and every q is an integer."""
    k = np.random.default_rng(seed).integers(0, 64, size=(24, 40))
    d = (-(1.0 + k / 64.0)).astype(np.float32)
    d.setflags(write=False)
    return d, k


@functools.lru_cache(maxsize=None)
def tie_map_dense(seed=6):
    """The same quantum, with neighbours 3, 4 or 5 quanta apart (a checkerboard of +-4 plus a random 0 / 1): here the exact tie
    |delta| == max_jump decides whether a pixel HAS a normal, which the sparse ties of tie_map() hardly ever do."""
    yy, xx = np.mgrid[0:24, 0:40]
    k = 30 + 4 * ((xx + yy) % 2) + (np.random.default_rng(seed).random((24, 40)) < 0.25)
    d = (-(1.0 + k / 64.0)).astype(np.float32)
    d.setflags(write=False)
    return d, k


def tie_tables(radius):
    sp, _, _ = tables_np(radius)
    lut = np.exp(-np.arange(TIE_NLUT, dtype=np.float64) / 64.0).astype(np.float32)   # any table will do: each entry is distinct
    return sp, lut, TIE_SCALE
