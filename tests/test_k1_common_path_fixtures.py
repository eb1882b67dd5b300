"""CPU: the fixtures of tests/k1_common_path_cases.py hold the classes they claim where there is no GPU -- counted from the numpy
oracle's chain alone -- the two oracles agree on them bit for bit, and no voxel sits near enough to the guard band for the
counts to depend on how the band is evaluated."""
import numpy as np
import pytest

import k1_common_path_cases as C
from oracle import oracle_c as OC
from oracle import oracle_np as O


@pytest.fixture(scope="module", autouse=True)
def _built():
    OC.build()


@pytest.mark.parametrize("case", C.CASES, ids=[c["name"] for c in C.CASES])
def test_cases_hold_their_classes_and_the_oracles_agree(case):
    c = case
    counts = C.classes(c)
    print(c["name"], {k: v for k, v in counts.items() if v})
    for name in c["claims"]:
        assert counts[name] > 0, (name, counts)
    assert counts["unsure_voxels"] == 0, counts
    assert c["res"] in C.GRIDS.values() and len(c["views"]) >= 2
    assert all(dm.shape[0] <= 48 and dm.shape[1] <= 64 for _, dm in c["views"])
    kw = dict(tsdf_res=c["tsdf_res"], scale=c["scale"], center=c["center"], wmax=3.0)
    Tn, Wn = np.zeros(c["res"]) + c["tdist"], np.zeros(c["res"])
    Tc, Wc = Tn.copy(), Wn.copy()
    margin, updated = [None], 0
    for lw, dm in c["views"]:
        _, _, mask = O.fuse_depths(dm, lw, c["K"], c["Kinv"], Tn, Wn, c["tdist"], margin_out=margin, return_mask=True, **kw)
        n = OC.fuse_depths(dm, lw, c["K"], c["Kinv"], Tc, Wc, c["tdist"], **kw)
        assert n == int(mask.sum())
        updated += n
        assert np.array_equal(dm.astype(np.float32).astype(np.float64), dm)        # float32 maps hold the same values
    assert np.array_equal(Wn, Wc) and np.array_equal(Tn, Tc)
    assert 0 < updated < 2 * Wn.size
    if c["margin_zero"]:
        assert margin[0] == 0.0


def test_every_class_of_the_issue_is_claimed_on_both_grids():
    for grid in C.GRIDS:
        claimed = {name for c in C.CASES if c["name"].endswith("-" + grid) for name in c["claims"]}
        assert claimed == set(C.classes(C.CASES[0])) - {"unsure_voxels"}, (grid, claimed)
