"""CPU: the band-sample definition of include/dfusion_hip.h restated in numpy (tests/extract_np.py) against
pipeline.extract_surface_samples_torch on CPU tensors -- identical voxel sets in identical order, positions and normals to
1e-12 (the torch statement takes its norm with torch.norm, not sqrt((gx gx + gy gy) + gz gz): an ulp or two) -- and the rule
itself on the planted volumes of tests/extract_cases.py: exact band ties, weights that are 0 / negative / NaN / subnormal, the
|gradient| gate 1 % either side of 1e-6, NaN and infinite neighbours."""
import numpy as np
import pytest
import torch

import extract_cases as EC
import extract_np as EN
from dynamicfusion_body_amd.pipeline import extract_surface_samples_torch

TOL = 1e-12


def against_torch(T, W, band, x0=0, capacity=None):
    pos, nrm, vox, total = EN.band_samples(T, W, band, x0=x0, capacity=capacity)
    pt, nt = extract_surface_samples_torch(torch.from_numpy(T), torch.from_numpy(W), band, x0=x0, max_samples=capacity)
    pt, nt = pt.numpy(), nt.numpy()
    assert pt.shape == pos.shape and nt.shape == nrm.shape
    assert np.isfinite(pt).all() and np.isfinite(nt).all() and np.isfinite(pos).all() and np.isfinite(nrm).all()
    assert np.array_equal(EN.voxel_of(pt, nt, T, vox, x0), vox)
    if len(pos):
        assert np.abs(pt - pos).max() <= TOL and np.abs(nt - nrm).max() <= TOL
    return pos, nrm, vox, total


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", EC.SHAPES)
def test_noise_volumes(shape, dtype):
    T, W = EC.noise(shape, dtype, seed=sum(shape))
    for x0 in (0, 13):
        pos, nrm, vox, total = against_torch(T, W, EC.BAND, x0=x0)
        assert total == len(pos) and total >= np.prod(shape) // 4
        assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() < 1e-14
        # the step is no longer than |T|: a sample stays within the band of its voxel's centre
        assert (np.linalg.norm(pos - (vox + [x0, 0, 0]), axis=1) <= np.abs(T[tuple(vox.T)].astype(np.float64)) + TOL).all()
    for cap in (0, 1, total // 3, total - 1, total, total + 5):
        sub, _, svox, t2 = against_torch(T, W, EC.BAND, x0=13, capacity=cap)
        assert t2 == total and len(sub) == min(cap, total)
        if 0 < cap < total:                                               # sample ceil(slot * total / cap) of the full list, per slot
            sel = [-((-s * total) // cap) for s in range(cap)]
            assert np.array_equal(svox, vox[sel]) and np.array_equal(sub, pos[sel])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dense_band_every_voxel_is_a_sample(dtype):
    T, W = EC.dense(dtype)
    pos, nrm, vox, total = against_torch(T, W, 10.0)
    assert total == T.size
    assert np.array_equal(vox, np.argwhere(np.ones(T.shape, dtype=bool)))        # voxel order


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planted_ties_weights_gate_and_bad_values(dtype):
    cases = EC.planted(dtype)
    assert len(cases) >= 15
    for case in cases:
        pos, nrm, vox, total = against_torch(case.T, case.W, case.band, x0=3)
        EC.check_case(case, vox, total)


def test_the_4_cubed_volume_with_one_infinite_voxel():
    """One +inf voxel in a 4^3 float32 volume: without the finiteness rule its six neighbours were samples with NaN rows
    (63 samples, 6 of them NaN); with it they are no samples."""
    T = (0.25 * np.arange(64, dtype=np.float32).reshape(4, 4, 4) / 16.0).astype(np.float32)
    T[1, 2, 1] = np.inf
    W = np.ones_like(T)
    pos, nrm, vox, total = against_torch(T, W, 1.5)
    assert total == 64 - 1 - 6
    assert not ({(1, 2, 1), (0, 2, 1), (2, 2, 1), (1, 1, 1), (1, 3, 1), (1, 2, 0), (1, 2, 2)} & set(map(tuple, vox.tolist())))
