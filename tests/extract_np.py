"""TEST INFRASTRUCTURE ONLY: the band-voxel sample definition of include/dfusion_hip.h (dfh_surface_count / dfh_surface_emit,
csrc/dfh_extract.hip) restated in plain fp64 numpy, in the operation order the header gives.  numpy only: neither torch nor the
library is imported here, so this is a definition to compare both against, not a third implementation sharing their code.

A voxel (x, y, z) of a volume T (X, Y, Z) with weights W is a sample iff
    (double)W > 0  and  |(double)T| < band                     (both strict, both false for NaN)
and the length of its gradient is finite and > 1e-6, where
    g_a = (T[hi] - T[lo]) / (hi - lo),  lo = max(i - 1, 0), hi = min(i + 1, n - 1)   along each axis a; 0 where n == 1
    n   = sqrt((gx * gx + gy * gy) + gz * gz)
Then   nrm = g / n,   st = t / max(n, 1),   pos = (centre with x0 added to its first coordinate) - st * nrm.
Samples come in voxel order (C order of the array).  capacity < total keeps an even subsample: sample i belongs to slot
floor(i * capacity / total) and is kept iff it is the first of its slot."""
import numpy as np


def _diff(Td, i, n, take):
    lo, hi = np.maximum(i - 1, 0), np.minimum(i + 1, n - 1)
    d = hi - lo
    return np.where(d > 0, (take(hi) - take(lo)) / np.maximum(d, 1).astype(np.float64), 0.0)


def band_samples(T, W, band, x0=0, capacity=None):
    """-> pos (S,3) f64, nrm (S,3) f64, vox (S,3) int64 (the voxel of every sample, local indices), total (samples before the
    capacity rule)."""
    T, W = np.asarray(T), np.asarray(W)
    assert T.ndim == 3 and W.shape == T.shape
    X, Y, Z = T.shape
    Td, Wd = T.astype(np.float64), W.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ix, iy, iz = np.nonzero((Wd > 0.0) & (np.abs(Td) < float(band)))          # C order = voxel order
        gx = _diff(Td, ix, X, lambda a: Td[a, iy, iz])
        gy = _diff(Td, iy, Y, lambda a: Td[ix, a, iz])
        gz = _diff(Td, iz, Z, lambda a: Td[ix, iy, a])
        n = np.sqrt((gx * gx + gy * gy) + gz * gz)
        ok = np.isfinite(n) & (n > 1e-6)
    ix, iy, iz, gx, gy, gz, n = (a[ok] for a in (ix, iy, iz, gx, gy, gz, n))
    total = len(n)
    if capacity is not None and capacity < total:
        cap = int(capacity)
        slot = np.array([(i * cap) // total for i in range(total)], dtype=np.int64)  # (python integers: no overflow)
        keep = np.ones(total, dtype=bool)
        keep[1:] = slot[1:] != slot[:-1]
        if cap == 0:
            keep[:] = False
        ix, iy, iz, gx, gy, gz, n = (a[keep] for a in (ix, iy, iz, gx, gy, gz, n))
    t = Td[ix, iy, iz]
    nrm = np.stack([gx / n, gy / n, gz / n], axis=1)
    st = t / np.maximum(n, 1.0)
    centre = np.stack([(ix + int(x0)).astype(np.float64), iy.astype(np.float64), iz.astype(np.float64)], axis=1)
    pos = centre - st[:, None] * nrm
    vox = np.stack([ix, iy, iz], axis=1).astype(np.int64)
    return pos, nrm, vox, total


def voxel_of(pos, nrm, T, vox, x0=0):
    """The voxel every (pos, nrm) row of another implementation came from, given the restatement's voxel list `vox` of the same
    length: centre = pos + st * nrm with the restatement's own step st for row i, rounded.  Rows from another voxel than vox[i]
    come back as another voxel (or as garbage), which is all the caller compares."""
    T = np.asarray(T).astype(np.float64)
    X, Y, Z = T.shape
    ix, iy, iz = vox[:, 0], vox[:, 1], vox[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        gx = _diff(T, ix, X, lambda a: T[a, iy, iz])
        gy = _diff(T, iy, Y, lambda a: T[ix, a, iz])
        gz = _diff(T, iz, Z, lambda a: T[ix, iy, a])
        n = np.sqrt((gx * gx + gy * gy) + gz * gz)
        st = T[ix, iy, iz] / np.maximum(n, 1.0)
        c = np.rint(np.asarray(pos) + st[:, None] * np.asarray(nrm))
    c[:, 0] -= x0
    return c.astype(np.int64)
