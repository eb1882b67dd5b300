"""CPU: the systems of tests/test_gpu_pcg_shapes.py (tests/pcg_cases.py) are what they claim to be -- conditions on the INPUTS
that keep the GPU comparison honest: the two numpy recurrences the device paths are compared with agree with each other far below
the GPU test's bar, ten iterations are nowhere near convergence (nothing passes because PCG has converged anyway), the systems are
well conditioned (the 1e-9 bar is a statement about the kernels, not about error growth), and the launch shapes, row widths and
diagonal positions the cases were made for are really there."""
import numpy as np
import pytest

import pcg_cases as C
from oracle import gn_np as G

NAMES = C.NAMES


@pytest.fixture(scope="module")
def CASES():
    return C.cases()


def _iterates(c, fn):
    out = []
    fn(c["N"], c["keys"], c["blocks"], c["Jtr"], max(C.ITERS), *c["lm"], iterates=out)
    return out


def test_every_family_of_the_table_is_there(CASES):
    assert tuple(c["name"] for c in CASES) == C.NAMES
    assert tuple(c["name"] for c in CASES if c["compare_converged"]) == C.CONVERGED_NAMES
    assert tuple(c["name"] for c in CASES if c["N"] <= 300) == C.SMALL_NAMES
    assert [c["N"] for c in CASES if c["family"] == "tiny"] == [1, 2, 8, 9, 10, 11]
    assert [c["N"] for c in CASES if c["family"] == "groups"] == [40, 41, 256, 257]
    assert [c["N"] for c in CASES if c["family"] == "wg64"] == [512, 513]
    assert [c["N"] for c in CASES if c["family"] in ("widths", "late_diagonal")] == [64, 64]
    assert [(c["N"], c["lm"]) for c in CASES if c["family"] == "starved"] == [(41, (0.0, 0.0)), (41, (1e-3, 1e-2))]
    assert [c["N"] for c in CASES if c["family"] == "zero_rhs"] == [41, 41]
    assert [c["N"] for c in CASES if c["family"] in ("big16", "beyond")] == [2050, 4100]
    assert len(set(NAMES)) == len(NAMES) == 20
    assert C.ITERS == (1, 2, 3, 4, 5, 10)


@pytest.mark.parametrize("name", NAMES)
def test_layout_is_the_devices(name):
    """CSR with ascending columns, one explicit diagonal block per row, symmetric, keys = row * N + col."""
    c = C.case(name)
    N, rp, col = c["N"], c["row_ptr"], c["col"]
    assert rp[0] == 0 and rp[-1] == len(col) == len(c["keys"]) == len(c["blocks"]) and len(rp) == N + 1
    rows = np.repeat(np.arange(N), np.diff(rp))
    assert np.array_equal(c["keys"], rows.astype(np.int64) * N + col) and np.all(np.diff(c["keys"]) > 0)
    assert np.array_equal(np.bincount(rows[col == rows], minlength=N), np.ones(N, dtype=np.int64))      # one diagonal block per row
    mirror = np.searchsorted(c["keys"], col.astype(np.int64) * N + rows)
    assert np.array_equal(c["keys"][mirror], col.astype(np.int64) * N + rows)
    assert np.array_equal(c["blocks"], np.transpose(c["blocks"][mirror], (0, 2, 1)))
    assert c["Jtr"].shape == (N, 6)


@pytest.mark.parametrize("name", NAMES)
def test_the_two_recurrences_agree_at_every_iteration_count(name):
    """pcg_cg1 (what the persistent kernel is compared with) and pcg_textbook (the multi-launch path): <= 1e-12 max|x|."""
    c = C.case(name)
    a, b = _iterates(c, G.pcg_cg1), _iterates(c, G.pcg_textbook)
    for k in C.ITERS:
        assert np.isfinite(a[k - 1]).all() and np.isfinite(b[k - 1]).all()
        assert np.abs(a[k - 1] - b[k - 1]).max() <= 1e-12 * np.abs(a[k - 1]).max(), (name, k)
        # `iterates` is what a run of k iterations returns
    assert np.array_equal(a[2], G.pcg_cg1(c["N"], c["keys"], c["blocks"], c["Jtr"], 3, *c["lm"]))
    assert np.array_equal(b[2], G.pcg_textbook(c["N"], c["keys"], c["blocks"], c["Jtr"], 3, *c["lm"]))


@pytest.mark.parametrize("name", C.CONVERGED_NAMES)
def test_ten_iterations_are_not_converged(name):
    c = C.case(name)
    assert c["N"] >= 40
    x10 = _iterates(c, G.pcg_cg1)[9]
    import scipy.sparse.linalg as spl
    A = G.blocks_to_bsr(c["N"], c["keys"], G.damp_blocks(c["N"], c["keys"], c["blocks"], *c["lm"])).tocsc()
    xs = spl.spsolve(A, -c["Jtr"].reshape(-1))
    assert np.abs(A @ xs + c["Jtr"].reshape(-1)).max() <= 1e-11 * np.abs(c["Jtr"]).max()
    assert np.abs(x10 - xs).max() >= 1e-4 * np.abs(xs).max()


def test_which_cases_are_compared_with_the_converged_solution(CASES):
    """Every non-degenerate case with N >= 40 is."""
    for c in CASES:
        degenerate = c["family"] in ("starved",) or c["name"] == "zero_rhs-all"
        assert c["compare_converged"] == (c["N"] >= 40 and not degenerate), c["name"]


@pytest.mark.parametrize("name", C.SMALL_NAMES)
def test_condition_number(name):
    c = C.case(name)
    ev = np.linalg.eigvalsh(C.dense(c))
    if "singular" in c["claims"]:
        assert name == "starved-undamped" and ev[0] <= 1e-12 * ev[-1]      # singular by design: compared iterate to iterate only
    else:
        assert ev[0] > 0.0 and ev[-1] / ev[0] <= 1e4


def test_widths_case_has_every_width_class():
    c = C.case("widths")
    w = C.widths(c)
    for node, width in C.WIDTH_CLAIMS.items():
        assert w[node] == width, (node, w[node])
    assert set(C.WIDTH_CLAIMS.values()) == {1, 10, 11, 30, 31, 63} and w.max() >= 48
    assert c["col"][c["row_ptr"][0]] == 0                                   # the isolated node's one block is its diagonal
    assert np.abs(c["blocks"][c["row_ptr"][0]]).max() > 0.0


def test_late_diagonals_are_beyond_the_register_cache(CASES):
    c = C.case("late_diagonal")
    assert {a: C.diagonal_position(c, a) for a in C.LATE_DIAGONALS} == C.LATE_DIAGONALS == {63: 63, 40: 35}
    assert min(C.LATE_DIAGONALS.values()) >= C.ROW_CACHE and c["lm"][0] > 0.0
    # every other case keeps the diagonal inside the cache, i.e. this case alone reaches the kernel's other branch
    for o in CASES:
        if o["name"] != "late_diagonal" and o["N"] <= 600:
            assert max(C.diagonal_position(o, a) for a in range(o["N"])) < C.ROW_CACHE, o["name"]


def test_starved_nodes():
    for name in ("starved-undamped", "starved-damped"):
        c = C.case(name)
        for a in C.STARVED_EMPTY:
            assert C.widths(c)[a] == 1 and not c["blocks"][c["row_ptr"][a]].any() and not c["Jtr"][a].any()
        d = c["blocks"][c["row_ptr"][C.STARVED_RANK1] + C.diagonal_position(c, C.STARVED_RANK1)]
        assert np.linalg.matrix_rank(d) == 1 and c["Jtr"][C.STARVED_RANK1].any()
        # exact zero pivots, not rounded ones: the undamped block's inverse under the pivot rule is exactly that of
        # L = I with the first column replaced by j / j[0]
        j = np.array([0.25, 0.5, -0.25, 0.125, -0.5, 0.375])
        assert np.array_equal(d, np.outer(j, j))
        L = np.eye(6); L[:, 0] = j
        Li = np.linalg.inv(L)
        assert np.abs(G.block_jacobi_inverse(d[None])[0] - Li.T @ Li).max() <= 1e-13 * np.abs(Li.T @ Li).max()
        # the oracle leaves the empty nodes' rows at exactly zero
        for x in _iterates(c, G.pcg_cg1) + _iterates(c, G.pcg_textbook):
            assert not x.reshape(-1, 6)[list(C.STARVED_EMPTY)].any()


def test_zero_rhs_cases():
    c = C.case("zero_rhs-all")
    assert not c["Jtr"].any() and c["blocks"].any()
    assert all(not x.any() for x in _iterates(c, G.pcg_cg1) + _iterates(c, G.pcg_textbook))
    p = C.case("zero_rhs-ten_rows")
    zero = ~p["Jtr"].any(axis=1)
    assert zero.sum() == 10 and np.array_equal(np.flatnonzero(zero), C.ZERO_RHS_ROWS)


def test_launch_shapes():
    """What N and the waves per workgroup imply: 64 against 65 workgroups, trailing waves without a row, the first automatic
    16-wave grid and the first grid beyond the persistent kernel (for a 256-CU device; the GPU test uses its own CU count)."""
    n_cu = 256
    assert C.workgroups(512, 8) == 64 and C.workgroups(513, 8) == 65
    assert C.workgroups(8, 8) == 1 and C.workgroups(9, 8) == 2 and 9 % 8 == 1            # seven waves without a row
    assert C.workgroups(1, 16) == 1 and C.workgroups(11, 4) == 3
    n16, nb = C.shape_sizes(n_cu)
    assert (n16, nb) == (2050, 4100) == (C.case("big16")["N"], C.case("beyond")["N"])
    assert C.auto_wpb(n16, n_cu) == 16 and C.auto_wpb(n16 - 2, n_cu) == 8 and C.workgroups(n16, 16) <= n_cu
    assert C.workgroups(nb, C.auto_wpb(nb, n_cu)) > n_cu                                  # no persistent grid fits
    assert (nb + 3) // 4 > 256 and (nb + 255) // 256 > 1                                  # > 256 partials, > 1 init workgroup
    # update_xr's groups: 10 nodes per wave, 40 per workgroup; pcg_init_kernel: 256 per workgroup
    assert [(N + 39) // 40 for N in (10, 11, 40, 41)] == [1, 1, 1, 2] and [(N + 255) // 256 for N in (256, 257)] == [1, 2]
