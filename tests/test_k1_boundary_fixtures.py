"""CPU: the exact-arithmetic K1 fixtures (tests/k1_boundary_cases.py) are what they claim to be where there is no GPU -- the numpy
oracle and the C oracle agree on them bit for bit, the oracle reports a margin of exactly 0, and every boundary class a case
claims holds at least MIN_CLASS voxels."""
import numpy as np
import pytest

import k1_boundary_cases as B
from oracle import oracle_c as OC
from oracle import oracle_np as O


@pytest.fixture(scope="module", autouse=True)
def _built():
    OC.build()


@pytest.mark.parametrize("case", B.EXACT_CASES, ids=[c["name"] for c in B.EXACT_CASES])
def test_exact_cases_sit_on_the_boundaries_and_the_oracles_agree(case):
    c = case
    counts = B.voxel_classes(c)
    print(c["name"], counts)
    for name in c["claims"]:
        assert counts[name] >= B.MIN_CLASS, (name, counts)
    kw = dict(tsdf_res=c["tsdf_res"], scale=c["scale"], center=c["center"], wmax=3.0)
    Tn, Wn = np.zeros(c["res"]) + c["tdist"], np.zeros(c["res"])
    Tc, Wc = Tn.copy(), Wn.copy()
    for rep in range(2):
        margin = [None]
        _, _, mask = O.fuse_depths(c["dm"], c["lw"], c["K"], c["Kinv"], Tn, Wn, c["tdist"], margin_out=margin, return_mask=True, **kw)
        assert margin[0] == 0.0
        n = OC.fuse_depths(c["dm"], c["lw"], c["K"], c["Kinv"], Tc, Wc, c["tdist"], **kw)
        assert n == int(mask.sum()) == counts["updated"]
        assert np.array_equal(mask, B.chain(c)["upd"])
        assert np.array_equal(Wn, Wc) and np.array_equal(Tn, Tc)
    assert 0 < counts["updated"] < Wn.size
    # float32 depth maps hold the same (dyadic) values
    assert np.array_equal(c["dm"].astype(np.float32).astype(np.float64), c["dm"])


def test_closed_form_inverse_is_exact():
    for c in B.EXACT_CASES:
        assert np.array_equal(c["K"] @ c["Kinv"], np.eye(3))
        assert tuple(c["Kinv"][2]) == (0.0, 0.0, 1.0)
    assert any(c["K"][0, 1] != 0 and c["K"][1, 1] != c["K"][0, 0] for c in B.EXACT_CASES)       # a general 3 x 3 K is among them
