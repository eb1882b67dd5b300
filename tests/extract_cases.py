"""TEST INFRASTRUCTURE ONLY: the volumes on which tests/test_extract_np.py (CPU, the torch definition) and
tests/test_gpu_extract_edges.py (the HIP kernels) are compared with tests/extract_np.py.  numpy only.

Every planted case says what the rule of include/dfusion_hip.h makes of it (`include` / `exclude`: voxels that must / must not
be samples; `exact`: the whole sample set, where the construction fixes it; `count`), so that the restatement itself is pinned
before anything is compared with it."""
from collections import namedtuple

import numpy as np

SHAPES = [(5, 3, 4), (2, 2, 8), (3, 1, 12), (4, 16, 16), (5, 5, 41), (3, 11, 31), (1, 6, 8)]
BAND = 1.5

Case = namedtuple("Case", "name T W band include exclude exact count")


def noise(shape, dtype, seed=0):
    """0.7 N(0,1), weights 1 with probability 0.8."""
    rng = np.random.default_rng(seed)
    T = (0.7 * rng.normal(size=shape)).astype(dtype)
    W = (rng.random(shape) < 0.8).astype(dtype)
    return T, W


def dense(dtype, shape=(4, 16, 64)):
    """T = 0.01 (x + 2y + 3z) rounded to dtype, all weights 1: with band 10 every voxel is a sample."""
    x, y, z = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij")
    return (0.01 * (x + 2.0 * y + 3.0 * z)).astype(dtype), np.ones(shape, dtype=dtype)


def ramp(dtype, shape=(5, 6, 8)):
    """0.3 x + 0.2 y + 0.1 z - 1: |gradient| = 0.37 everywhere, values from -1 to 1.9 (some outside the band of 1.5)."""
    x, y, z = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij")
    return (0.3 * x + 0.2 * y + 0.1 * z - 1.0).astype(dtype), np.ones(shape, dtype=dtype)


def _touched(bad):
    """voxels whose gradient reads a voxel of `bad`: its six neighbours (the clamped faces read the voxel itself)."""
    t = bad.copy()
    for a in range(3):
        b = np.moveaxis(bad, a, 0)
        tt = np.moveaxis(t, a, 0)
        tt[1:] |= b[:-1]
        tt[:-1] |= b[1:]
    return t


def _bad_value_case(name, dtype, plants):
    T, W = ramp(dtype)
    clean = (np.abs(T.astype(np.float64)) < BAND)
    for at, v in plants:
        T[at] = v
    gone = _touched(~np.isfinite(T))
    exact = clean & np.isfinite(T) & ~gone              # (the ramp's own gradient is 0.37: the gate passes wherever it is finite)
    return Case(name, T, W, BAND, [], [at for at, _ in plants], exact, None)


def planted(dtype):
    dtype = np.dtype(dtype)
    one = dtype.type(1)
    inside = np.nextafter(dtype.type(BAND), dtype.type(0))             # one ulp of the volume's type inside the band
    tiny = np.nextafter(dtype.type(0), one)                            # the smallest subnormal
    out = []
    # |T| == band: excluded (strict); one ulp inside: included
    T, W = ramp(dtype)
    T[2, 3, 4], T[2, 1, 2] = dtype.type(BAND), dtype.type(-BAND)
    T[1, 3, 5], T[3, 2, 1] = inside, -inside
    out.append(Case("band ties", T, W, BAND, [(1, 3, 5), (3, 2, 1)], [(2, 3, 4), (2, 1, 2)], None, None))
    # weights: 0, -1, NaN give no sample, the smallest subnormal does
    T, W = ramp(dtype)
    W[1, 1, 1], W[1, 1, 2], W[1, 1, 3], W[1, 1, 4] = 0, -1, np.nan, tiny
    W[4, 5, 0], W[0, 0, 7] = np.nan, tiny                              # (and at the two ends of the volume)
    out.append(Case("weights", T, W, BAND, [(1, 1, 4), (0, 0, 7)], [(1, 1, 1), (1, 1, 2), (1, 1, 3), (4, 5, 0)], None, None))
    # the gradient gate, 1 % either side of 1e-6, along each axis
    for axis in range(3):
        shape = (5, 6, 8)
        i = np.arange(shape[axis], dtype=np.float64).reshape([-1 if a == axis else 1 for a in range(3)])
        for slope, n in ((0.99e-6, 0), (1.01e-6, int(np.prod(shape)))):
            T = np.broadcast_to(slope * i, shape).astype(dtype)
            out.append(Case("ramp of %.2e along axis %d" % (slope, axis), T, np.ones(shape, dtype=dtype), BAND, [], [], None, n))
    # non-finite neighbours: no sample from any voxel whose gradient reads one, and none from the voxel itself
    out.append(_bad_value_case("NaN neighbour", dtype, [((2, 3, 4), np.nan)]))
    out.append(_bad_value_case("+inf neighbour", dtype, [((2, 3, 4), np.inf)]))
    out.append(_bad_value_case("-inf neighbour", dtype, [((1, 2, 3), -np.inf)]))
    out.append(_bad_value_case("inf on both sides (inf - inf)", dtype, [((2, 3, 3), np.inf), ((2, 3, 5), np.inf)]))
    out.append(_bad_value_case("+inf and -inf on both sides", dtype, [((2, 2, 4), np.inf), ((2, 4, 4), -np.inf)]))
    out.append(_bad_value_case("bad values in the corners and in the first and last pack of a row", dtype,
                               [((0, 0, 0), np.nan), ((4, 5, 7), np.inf), ((0, 5, 3), -np.inf), ((3, 0, 4), np.nan)]))
    # a finite neighbour so large that |gradient| overflows (fp64 volumes) is "not finite" too; FLT_MAX in an fp32 volume is
    # not: its square fits a double, the voxel is a sample with a finite position
    T, W = ramp(dtype)
    big = np.finfo(dtype).max
    T[2, 3, 4] = big
    if dtype == np.float64:
        out.append(Case("neighbour whose square overflows", T, W, BAND, [(0, 0, 0)], [(2, 3, 4), (2, 3, 3), (1, 3, 4), (2, 4, 4)], None, None))
    else:
        out.append(Case("FLT_MAX neighbour", T, W, BAND, [(2, 3, 3), (1, 3, 4), (2, 2, 4)], [(2, 3, 4)], None, None))
    return out


def check_case(case, vox, total):
    """What the construction says about the sample set `vox` (S,3)."""
    got = set(map(tuple, vox.tolist()))
    for at in case.include:
        assert tuple(at) in got, (case.name, "missing", at)
    for at in case.exclude:
        assert tuple(at) not in got, (case.name, "unexpected", at)
    if case.exact is not None:
        assert got == set(map(tuple, np.argwhere(case.exact).tolist())), case.name
        assert len(got) > 20, case.name
    if case.count is not None:
        assert total == case.count, (case.name, total)
