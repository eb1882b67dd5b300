"""GPU: band-voxel extraction (dfh_surface_count / dfh_surface_emit, csrc/dfh_extract.hip) against the numpy restatement of the
header's definition (tests/extract_np.py) at the structural edges of the kernels: z rows of one and two 16-byte packs, a
one-voxel-thick y axis, volumes of 1023 / 1024 / 1025 voxels (the 1024-voxel block), a band so wide that every voxel of every
block is a sample (the emit pass's wave prefixes at full load), the pack kernels against the scalar kernels on the same data,
exact band ties, weights that are 0 / negative / NaN / subnormal, the |gradient| gate 1 % either side of 1e-6, NaN and infinite
neighbours, and the C entry point's capacity handling behind guard words.

The sample count and the voxel of every sample must be exact; positions and normals agree to 1e-12 (fp64 arithmetic in the same
operation order: the bar tests/test_gpu_pipeline.py holds this kernel to)."""
import numpy as np
import pytest
import torch

import extract_cases as EC
import extract_np as EN
from dynamicfusion_body_amd import _lib
from dynamicfusion_body_amd.device import current_stream_ptr, dtype_code
from dynamicfusion_body_amd.pipeline import extract_surface_samples

pytestmark = pytest.mark.gpu

TOL = 1e-12


def dev(a, offset=0):
    """numpy array -> contiguous CUDA tensor; offset > 0: a view starting `offset` elements into a flat buffer (contiguous, but
    the base pointer is not 16-byte aligned: the float32 pack kernels cannot take it, the scalar kernels run)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if offset == 0:
        d = t.cuda().contiguous()
        assert d.data_ptr() % 16 == 0
        return d
    flat = torch.zeros(a.size + offset, dtype=t.dtype, device="cuda")
    d = flat[offset:].view(a.shape)
    d.copy_(t)
    assert d.is_contiguous() and d.data_ptr() % 16 != 0
    return d


def against_definition(T, W, band, x0=0, t_off=0, w_off=0):
    ref_pos, ref_nrm, vox, total = EN.band_samples(T, W, band, x0=x0)
    pos, nrm = extract_surface_samples(dev(T, t_off), dev(W, w_off), band, x0=x0)
    assert pos.shape == (total, 3) and nrm.shape == (total, 3), (pos.shape, total)
    p, n = pos.cpu().numpy(), nrm.cpu().numpy()
    assert np.isfinite(p).all() and np.isfinite(n).all()
    assert np.array_equal(EN.voxel_of(p, n, T, vox, x0), vox)
    if total:
        ep, en = np.abs(p - ref_pos).max(), np.abs(n - ref_nrm).max()
        assert ep <= TOL and en <= TOL, (ep, en)
    return pos, nrm, vox, total


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", EC.SHAPES)
def test_small_and_ragged_shapes(shape, dtype):
    """Z = 4 and Z = 8 (one and two packs per row, both z neighbours of a pack clamped), Y = 1, X = 1, 1023 / 1024 / 1025 voxels;
    (5,5,41) and (3,11,31) take the scalar float32 kernels, float64 the scalar kernels throughout."""
    T, W = EC.noise(shape, dtype, seed=sum(shape))
    for x0 in (0, 13):
        _, _, _, total = against_definition(T, W, EC.BAND, x0=x0)
        assert total >= np.prod(shape) // 4


@pytest.mark.parametrize("dtype,off", [(np.float32, 0), (np.float32, 1), (np.float64, 0)])
def test_dense_band_every_voxel_is_a_sample(dtype, off):
    """Four blocks in which every thread emits all four of its voxels, on the pack path and on the scalar path."""
    T, W = EC.dense(dtype)
    _, _, vox, total = EN.band_samples(T, W, 10.0)
    assert total == T.size and np.array_equal(vox, np.argwhere(np.ones(T.shape, dtype=bool)))
    pos, _, _, total = against_definition(T, W, 10.0, t_off=off, w_off=off)
    assert total == T.size


@pytest.mark.parametrize("shape", [(6, 7, 8), (9, 5, 44), (40, 33, 48)])
def test_pack_kernels_and_scalar_kernels_give_the_same_bits(shape):
    """ "The same doubles, the same decisions, the same samples": float32 data once aligned (pack kernels) and once behind a
    misaligned base of T, of Wt and of both (scalar kernels)."""
    T, W = EC.noise(shape, np.float32, seed=shape[0])
    pos, nrm, _, total = against_definition(T, W, EC.BAND, x0=5)
    assert total > np.prod(shape) // 4
    for t_off, w_off in ((1, 0), (0, 1), (1, 1), (3, 2)):
        p2, n2 = extract_surface_samples(dev(T, t_off), dev(W, w_off), EC.BAND, x0=5)
        assert torch.equal(p2, pos) and torch.equal(n2, nrm), (t_off, w_off)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planted_ties_weights_gate_and_bad_values(dtype):
    """The rule of the header where it is sharp; every case on the pack path (float32, aligned) and on the scalar path."""
    for case in EC.planted(dtype):
        for off in ((0, 1) if dtype == np.float32 else (0,)):
            _, _, vox, total = against_definition(case.T, case.W, case.band, x0=3, t_off=off, w_off=off)
            EC.check_case(case, vox, total)


@pytest.mark.parametrize("dtype,shape", [(np.float32, (9, 5, 44)), (np.float64, (5, 5, 41))])
def test_c_entry_point_capacities_behind_guard_words(dtype, shape):
    """dfh_surface_emit writes exactly min(total, capacity) rows -- the even subsample for capacity < total -- and nothing
    behind them; capacity 0 needs no output arrays."""
    lib = _lib.load()
    T, W = EC.noise(shape, dtype, seed=7)
    Td, Wd = dev(T), dev(W)
    res = _lib.iarr(shape)
    nbytes = lib.dfh_surface_workspace_bytes(res)
    ws = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device="cuda")
    tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    _lib.check(lib.dfh_surface_count(Td.data_ptr(), Wd.data_ptr(), dtype_code(Td), res, EC.BAND, ws.data_ptr(), nbytes, tot.data_ptr(),
                                     current_stream_ptr()), "dfh_surface_count")
    total = int(tot.item())
    assert total == EN.band_samples(T, W, EC.BAND)[3] and total > 100
    guard, sentinel = 9, -7.5
    for cap in (0, 1, total - 1, total, total + 5):
        rows = min(total, cap)
        pos = torch.full((3 * max(cap, 1) + guard,), sentinel, dtype=torch.float64, device="cuda")
        nrm = torch.full((3 * max(cap, 1) + guard,), sentinel, dtype=torch.float64, device="cuda")
        null = cap == 0
        _lib.check(lib.dfh_surface_emit(Td.data_ptr(), Wd.data_ptr(), dtype_code(Td), res, 2, EC.BAND, ws.data_ptr(),
                                        None if null else pos.data_ptr(), None if null else nrm.data_ptr(), cap, current_stream_ptr()),
                   "dfh_surface_emit")
        ref_pos, ref_nrm, _, _ = EN.band_samples(T, W, EC.BAND, x0=2, capacity=cap)
        assert len(ref_pos) == rows
        p, n = pos.cpu().numpy(), nrm.cpu().numpy()
        assert (p[3 * rows:] == sentinel).all() and (n[3 * rows:] == sentinel).all(), cap
        if rows:
            assert np.abs(p[:3 * rows].reshape(-1, 3) - ref_pos).max() <= TOL and np.abs(n[:3 * rows].reshape(-1, 3) - ref_nrm).max() <= TOL
