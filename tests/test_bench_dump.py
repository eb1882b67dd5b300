"""CPU: bench.py --dump-outputs (bench.dump_outputs) on host tensors -- what it writes, that the voxel sample is fixed, that it
stays within 64 MB, and that the per-rank slab files concatenate to the one-rank files."""
import os

import numpy as np
import torch

import bench


def _load(d, name):
    return np.load(os.path.join(d, name + ".npy"))


def test_small_grid_is_written_whole(tmp_path):
    T = torch.rand(32, 24, 16)
    W = torch.rand(32, 24, 16) * 100
    info = bench.dump_outputs(torch, str(tmp_path), T, W, T.numel(), (0, 32), 24 * 16, 0, 1)
    assert info["files"] == ["tsdf.npy", "weight.npy"] and info["sample"] is None
    for name, v in (("tsdf", T), ("weight", W)):
        a = _load(str(tmp_path), name)
        assert a.dtype == np.float32 and np.array_equal(a, v.numpy())


def test_large_grid_sample_is_fixed_bounded_and_split_by_slab(tmp_path):
    X, Y, Z = 170, 160, 160                                    # more voxels than DUMP_VOXELS: a sample is written
    n = X * Y * Z
    T = torch.arange(n, dtype=torch.float64).reshape(X, Y, Z)  # (the value is the flat index: exact in float64)
    W = -T
    one, again = str(tmp_path / "one"), str(tmp_path / "again")
    info = bench.dump_outputs(torch, one, T, W, n, (0, X), Y * Z, 0, 1)
    bench.dump_outputs(torch, again, T, W, n, (0, X), Y * Z, 0, 1)
    idx = _load(one, "tsdf")
    assert info["sample"] == {"of_voxels": n, "seed": bench.DUMP_SEED}
    assert idx.dtype == np.float32 and idx.shape == (bench.DUMP_VOXELS,)
    assert np.all(np.diff(idx.astype(np.int64)) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(_load(one, "weight"), -idx)
    assert sum(os.path.getsize(os.path.join(one, f)) for f in info["files"]) <= 64 << 20
    for name in ("tsdf", "weight"):
        assert np.array_equal(_load(one, name), _load(again, name))
    three = str(tmp_path / "three")
    cuts = (0, 57, 113, X)
    for r in range(3):
        a, b = cuts[r], cuts[r + 1]
        info = bench.dump_outputs(torch, three, T[a:b], W[a:b], n, (a, b), Y * Z, r, 3)
        assert info["files"] == ["tsdf.rank%d.npy" % r, "weight.rank%d.npy" % r]
    for name in ("tsdf", "weight"):
        parts = [_load(three, "%s.rank%d" % (name, r)) for r in range(3)]
        assert np.array_equal(np.concatenate(parts), _load(one, name))
