"""GPU: both block-Jacobi PCG paths (dfh_pcg_solve / dfh_pcg_solve_update through the C ABI) at every launch shape, row width and
iteration count, against the fp64 restatements oracle/gn_np.py pcg_cg1 (persistent single-reduction kernel) and pcg_textbook
(two launches per iteration).  The systems are tests/pcg_cases.py; tests/test_pcg_cases.py proves on the CPU that they reach the
shapes they claim, that the two oracles agree to 1e-12 on them and that ten iterations are far from converged.

The bar between a device path and its oracle is 1e-9 max|x_oracle| -- the bar test_gpu_solve.py uses between the two device
paths.  Measured worst deviations (MI355X, profiles/r8_pcg_shape_tests.txt): a few 1e-15 on every case, path and iteration count.

Every solve here runs with x_out and the workspace inside larger buffers of a fixed bit pattern (a quiet NaN with a payload): the
workspace is exactly dfh_pcg_workspace_bytes(N, iters) bytes, the margins must come back untouched, and what the solve does not
clear itself it meets as NaN.  dfh_pcg_status must report no timed-out solve."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pcg_cases as C
from oracle import gn_np as G
from dynamicfusion_body_amd import _lib
from dynamicfusion_body_amd.device import current_stream_ptr

pytestmark = pytest.mark.gpu

NAMES = C.NAMES
BAR = 1e-9
SENTINEL = 0x7FF85A5A5A5A5A5A                   # as a double: a quiet NaN
MARGIN = 512                                    # doubles (4 KiB) on either side
OPTIONS = ("pcg_multilaunch", "pcg_wpb")


@functools.lru_cache(maxsize=None)
def n_cu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def case(name):
    return C.case(name, n_cu())


@pytest.fixture(autouse=True)
def pcg_mode_auto():
    """Mode 0 (an earlier test of the process may have left 2: WarpSolver sets it for ranks that share a GPU, the time-out
    test's fall-back does), put back afterwards; the options a test set are cleared whatever happens."""
    lib = _lib.load()
    for o in OPTIONS:
        _lib.set_option(o, None)
    before = 2 if lib.dfh_pcg_path(8) == 2 else 0        # (8 rows: one workgroup, persistent unless the mode forbids it)
    _lib.check(lib.dfh_pcg_set_mode(0), "dfh_pcg_set_mode")
    try:
        yield lib
    finally:
        for o in OPTIONS:
            _lib.set_option(o, None)
        lib.dfh_pcg_set_mode(before)


class Guarded:
    """n doubles between two margins of the sentinel pattern; the payload starts as the pattern too."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * MARGIN,), SENTINEL, dtype=torch.int64, device="cuda")
        self.data = self.buf[MARGIN:MARGIN + n].view(torch.float64)

    def intact(self):
        return bool((self.buf[:MARGIN] == SENTINEL).all()) and bool((self.buf[MARGIN + self.n:] == SENTINEL).all())


def workspace(lib, N, iters):
    nbytes = lib.dfh_pcg_workspace_bytes(N, iters)
    assert nbytes > 0 and nbytes % 8 == 0
    return Guarded(nbytes // 8), nbytes


@functools.lru_cache(maxsize=None)
def device_system(name):
    c = case(name)
    return (torch.from_numpy(c["row_ptr"]).cuda(), torch.from_numpy(c["col"]).cuda(),
            torch.from_numpy(np.ascontiguousarray(c["blocks"])).cuda(), torch.from_numpy(np.ascontiguousarray(c["Jtr"])).cuda())


@functools.lru_cache(maxsize=None)
def oracle_iterates(name, path):
    c = case(name)
    out = []
    (G.pcg_cg1 if path == 1 else G.pcg_textbook)(c["N"], c["keys"], c["blocks"], c["Jtr"], max(C.ITERS), *c["lm"], iterates=out)
    for x in out:
        x.setflags(write=False)
    return out


def set_shape(lib, N, run):
    """run = ("multilaunch" | "persistent" | "auto", waves per workgroup or None).  Sets the options and returns the path
    dfh_pcg_path promises (asserted to be the intended one)."""
    kind, wpb = run
    _lib.set_option("pcg_multilaunch", 1 if kind == "multilaunch" else None)
    _lib.set_option("pcg_wpb", wpb)
    path = lib.dfh_pcg_path(N)
    if kind != "auto":
        assert path == (2 if kind == "multilaunch" else 1), (N, run, path)
    return path


def shapes(N):
    """The multi-launch path, the automatic shape, and every forced workgroup size whose grid fits one workgroup per CU."""
    runs = [("multilaunch", None)]
    if C.workgroups(N, C.auto_wpb(N, n_cu())) <= n_cu():
        runs.append(("persistent", None))
    else:
        runs.append(("auto", None))
    runs += [("persistent", w) for w in (4, 8, 16) if C.workgroups(N, w) <= min(n_cu(), 512)]
    return runs


def solve(lib, name, iters, run, rhs=None, ws=None, dq=None, step=1.0, expect_finite=True):
    """One solve of the case from a fresh copy of its matrix.  Returns (x, vals afterwards, path); the margins of x_out and of
    the workspace and the time-out counter are checked here."""
    c = case(name)
    N = c["N"]
    rp, cl, vals0, rhs0 = device_system(name)
    vals = vals0.clone()
    rh = rhs0 if rhs is None else rhs
    path = set_shape(lib, N, run)
    nbytes = lib.dfh_pcg_workspace_bytes(N, iters)
    if ws is None:
        ws, _ = workspace(lib, N, iters)
    assert ws.n * 8 >= nbytes
    x = Guarded(6 * N)
    args = (rp.data_ptr(), cl.data_ptr(), vals.data_ptr(), rh.data_ptr(), N, iters, c["lm"][0], c["lm"][1], x.data.data_ptr(),
            ws.data.data_ptr(), nbytes)
    if dq is None:
        _lib.check(lib.dfh_pcg_solve(*args, current_stream_ptr()), "dfh_pcg_solve")
    else:
        _lib.check(lib.dfh_pcg_solve_update(*args, dq.data_ptr(), step, current_stream_ptr()), "dfh_pcg_solve_update")
    aborted = ctypes.c_long(-1)
    _lib.check(lib.dfh_pcg_status(current_stream_ptr(), ctypes.byref(aborted)), "dfh_pcg_status")
    assert aborted.value == 0
    assert x.intact() and ws.intact(), (name, iters, run)
    xo = x.data.cpu().numpy()
    if expect_finite:
        assert np.isfinite(xo).all(), (name, iters, run)
    return xo, vals.cpu().numpy(), path


def check_matrix(c, vals):
    """The damping is written into the diagonal blocks' diagonals -- exactly damp_blocks -- and nothing else is touched."""
    assert np.array_equal(vals, G.damp_blocks(c["N"], c["keys"], c["blocks"], *c["lm"]))
    off = c["keys"] // c["N"] != c["keys"] % c["N"]
    assert np.array_equal(vals[off].view(np.int64), c["blocks"][off].view(np.int64))


def rel_dev(x, xo):
    scale = np.abs(xo).max()
    d = np.abs(x - xo).max()
    return d / scale if scale > 0.0 else d


@pytest.mark.parametrize("name", NAMES)
def test_iterates_on_every_path_and_shape(pcg_mode_auto, name):
    """x after 1, 2, 3, 4, 5 and 10 iterations (one reduction without a fetch; below the ring's first wrap and first clearing; past
    them) on the multi-launch path, the automatic shape and every forced workgroup size (4, 8, 16 waves) that fits the device,
    against the path's own recurrence in numpy; the matrix afterwards; and the persistent kernel twice for the same bits."""
    lib = pcg_mode_auto
    c = case(name)
    N = c["N"]
    if c["family"] == "wg64":
        if n_cu() < 65:
            pytest.skip("65 workgroups of 8 waves need 65 CUs; the device has %d" % n_cu())
        assert (C.workgroups(N, 8), N) in ((64, 512), (65, 513)) and ("persistent", 8) in shapes(N)
    runs = shapes(N)
    if c["family"] == "big16":
        assert N == 8 * n_cu() + 2 and C.auto_wpb(N, n_cu()) == 16 and ("persistent", None) in runs and ("persistent", 8) not in runs
    if c["family"] == "beyond":
        assert N == 16 * n_cu() + 4 and runs == [("multilaunch", None), ("auto", None)]
        assert (N + 3) // 4 > 256 and (N + 255) // 256 > 1
    if N <= 64:
        assert [w for k, w in runs if k == "persistent"] == [None, 4, 8, 16]
    if c["family"] == "widths":
        assert {node: int(C.widths(c)[node]) for node in C.WIDTH_CLAIMS} == C.WIDTH_CLAIMS
    if c["family"] == "late_diagonal":
        assert {a: C.diagonal_position(c, a) for a in C.LATE_DIAGONALS} == C.LATE_DIAGONALS
        assert min(C.LATE_DIAGONALS.values()) >= C.ROW_CACHE and c["lm"][0] > 0.0
    for run in runs:
        worst = []
        for iters in C.ITERS:
            x, vals, path = solve(lib, name, iters, run)
            if run[0] == "auto":
                assert path == 2                                    # no persistent grid fits: the automatic fall-back
            xo = oracle_iterates(name, path)[iters - 1]
            worst.append(rel_dev(x, xo))
            check_matrix(c, vals)
            if path == 1:
                x2, vals2, _ = solve(lib, name, iters, run)
                assert np.array_equal(x.view(np.int64), x2.view(np.int64)), (name, run, iters)
                assert np.array_equal(vals.view(np.int64), vals2.view(np.int64))
        print("pcg-shapes %-18s N=%5d %-11s wpb=%-4s path=%d  " % (name, N, run[0], run[1], path) +
              " ".join("it%d:%.1e" % (k, w) for k, w in zip(C.ITERS, worst)))
        for iters, w in zip(C.ITERS, worst):
            xo = oracle_iterates(name, path)[iters - 1]
            assert w <= (BAR if np.abs(xo).max() > 0.0 else 0.0), (name, run, iters, w)


@pytest.mark.parametrize("run", [("multilaunch", None), ("persistent", None), ("persistent", 4), ("persistent", 16)])
def test_zero_right_hand_side(pcg_mode_auto, run):
    """rhs = 0: every published value is an exact zero, which the persistent kernel stores as -0.0 so that the slot reads as
    "arrived"; gamma = delta = 0 takes the zero guards.  x is exactly zero, the twist update leaves node_dq as it is."""
    lib = pcg_mode_auto
    N = case("zero_rhs-all")["N"]
    dq0 = unit_dqs(N, 3)
    for iters in (1, 3, 10):
        x, vals, path = solve(lib, "zero_rhs-all", iters, run)
        assert np.array_equal(x, np.zeros(6 * N))
        check_matrix(case("zero_rhs-all"), vals)
        dq = torch.from_numpy(dq0).cuda()
        xu, _, _ = solve(lib, "zero_rhs-all", iters, run, dq=dq, step=1.0)
        assert np.array_equal(xu, np.zeros(6 * N))
        assert np.array_equal(dq.cpu().numpy(), dq0)
        # zero on ten rows only: those rows publish exact zeros in the first phase, the others do not
        xp, _, _ = solve(lib, "zero_rhs-ten_rows", iters, run)
        xo = oracle_iterates("zero_rhs-ten_rows", path)[iters - 1]
        assert np.abs(xp - xo).max() <= BAR * np.abs(xo).max()


@pytest.mark.parametrize("name", ["starved-undamped", "starved-damped"])
@pytest.mark.parametrize("run", [("multilaunch", None), ("persistent", None), ("persistent", 16)])
def test_starved_and_rank_deficient_blocks(pcg_mode_auto, name, run):
    """Nodes without a sample (all-zero diagonal block: every Cholesky pivot is 0 and becomes 1) and a node with one sample
    (rank-1 block), undamped and damped: finite, the empty nodes' rows exactly zero, and the oracle's iterates -- whose
    preconditioner follows the same pivot rule."""
    lib = pcg_mode_auto
    c = case(name)
    for iters in C.ITERS:
        x, vals, path = solve(lib, name, iters, run)
        assert np.isfinite(x).all()
        assert not x.reshape(-1, 6)[list(C.STARVED_EMPTY)].any()
        assert x.reshape(-1, 6)[C.STARVED_RANK1].any()
        xo = oracle_iterates(name, path)[iters - 1]
        assert np.abs(x - xo).max() <= BAR * np.abs(xo).max(), (name, run, iters)
        check_matrix(c, vals)


def unit_dqs(N, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(G.twist_exp_dq(rng.standard_normal((N, 6)) * np.array([0.6, 0.6, 0.6, 1.5, 1.5, 1.5])))


@pytest.mark.parametrize("name", ["groups-41", "big16"])
@pytest.mark.parametrize("kind", ["multilaunch", "persistent"])
def test_solve_update_is_the_solve_and_the_twists(pcg_mode_auto, name, kind):
    """dfh_pcg_solve_update: x_out has the bits of dfh_pcg_solve on the same path, node_dq <- exp(step x) (x) node_dq."""
    lib = pcg_mode_auto
    N = case(name)["N"]
    dq0 = unit_dqs(N, 8)
    assert np.abs(np.sum(dq0[:, :4] ** 2, axis=1) - 1.0).max() < 1e-14 and np.abs(dq0[:, 1:]).min() > 0.0
    x, _, path = solve(lib, name, 10, (kind, None))
    for step in (1.0, 0.5):
        dq = torch.from_numpy(dq0).cuda()
        xu, _, path_u = solve(lib, name, 10, (kind, None), dq=dq, step=step)
        assert path_u == path == (2 if kind == "multilaunch" else 1)
        assert np.array_equal(x.view(np.int64), xu.view(np.int64))
        want = G.apply_twists(dq0, step * x.reshape(N, 6))
        assert np.abs(dq.cpu().numpy() - want).max() <= 1e-12


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("run", [("multilaunch", None), ("persistent", None)])
def test_non_finite_rhs_leaves_node_dq_untouched(pcg_mode_auto, run, bad):
    """The header's contract for dfh_pcg_solve_update on BOTH paths: the twist update is all or nothing and happens only if
    every x is finite.  One NaN (or one +inf) in rhs: x_out is non-finite, node_dq keeps its bits, no solve counts as timed
    out, and the next solve in the same workspace with the clean rhs is the oracle's."""
    lib = pcg_mode_auto
    name = "groups-41"
    c = case(name)
    N = c["N"]
    rhs = device_system(name)[3].clone()
    rhs[17, 2] = bad
    dq0 = unit_dqs(N, 9)
    dq = torch.from_numpy(dq0).cuda()
    ws, _ = workspace(lib, N, 10)
    x, _, path = solve(lib, name, 10, run, rhs=rhs, ws=ws, dq=dq, step=1.0, expect_finite=False)   # (asserts: no time-out)
    assert not np.isfinite(x).any()
    assert np.array_equal(dq.cpu().numpy().view(np.int64), dq0.view(np.int64))
    x, _, _ = solve(lib, name, 10, run, ws=ws, dq=dq, step=1.0)
    xo = oracle_iterates(name, path)[9]
    assert np.abs(x - xo).max() <= BAR * np.abs(xo).max()
    assert np.abs(dq.cpu().numpy() - G.apply_twists(dq0, x.reshape(N, 6))).max() <= 1e-12


@pytest.mark.parametrize("run", [("multilaunch", None), ("persistent", None), ("persistent", 4)])
def test_workspace_reuse(pcg_mode_auto, run):
    """One workspace sized for 10 iterations: 10 iterations, then 3 (the hand-off ring and the partial slots sit at other
    offsets, over the first solve's leftovers), then a smaller system: each the bits of the same solve in a fresh workspace."""
    lib = pcg_mode_auto
    ws, _ = workspace(lib, 41, 10)
    for name, iters in (("groups-41", 10), ("groups-41", 3), ("tiny-9", 10), ("tiny-9", 2), ("groups-41", 10)):
        fresh, _, _ = solve(lib, name, iters, run)
        again, _, _ = solve(lib, name, iters, run, ws=ws)
        assert np.array_equal(fresh.view(np.int64), again.view(np.int64)), (name, iters)
    assert ws.intact()
