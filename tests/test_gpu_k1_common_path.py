"""K1's per-pack walk (view_pack) on the voxel classes that only few voxels fall into, brick by brick: near-surface voxels in one
slot of the four of a pack only, bricks with none / one / a near-surface voxel in every lane, a guard-band voxel beside a plain
near-surface one in one pack, single lanes with packs that straddle the camera plane, bricks outside the frustum, with one voxel
inside, or touching it only in the guard band of its edge (tests/k1_common_path_cases.py; the CPU twin,
tests/test_k1_common_path_fixtures.py, asserts the same counts from the oracle alone).

Every case runs through every sweep K1 has (check_all_sweeps of tests/test_gpu_k1_boundaries.py) under that module's bars: masks
and weights equal to the fp64 oracles, float32 values within 2 n eps32 (1 + |T|), every float32 sweep bit-identical to every
other.  Grids of 2 x 2 x 2 bricks (8 x 4 x 64) and a ragged 6 x 3 x 40, depth maps of at most 64 x 48, two views per case."""
import pytest
import torch

import k1_common_path_cases as C
from test_gpu_k1_boundaries import check_all_sweeps

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", C.CASES, ids=[c["name"] for c in C.CASES])
def test_every_sweep_on_the_rare_voxel_classes(case):
    c = case
    counts = C.classes(c)
    print(c["name"], {k: v for k, v in counts.items() if v})
    for name in c["claims"]:
        assert counts[name] > 0, (name, counts)
    assert counts["unsure_voxels"] == 0, counts
    To, Wo, masks, margin = check_all_sweeps(c["res"], c["tsdf_res"], c["K"], c["Kinv"], c["scale"], c["center"], c["tdist"], 3.0,
                                             c["views"], torch.float32)
    assert 0 < sum(int(m.sum()) for m in masks) < len(masks) * Wo.size
    if c["margin_zero"]:
        assert margin == 0.0
