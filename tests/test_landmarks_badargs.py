"""CPU: what dfh_gn_add_landmarks and dfh_gn_solve_landmarks do with arguments they cannot use, and with a term that adds nothing.
Validation comes before any HIP call, so no GPU is needed: device pointers are dummy non-null integers that nothing dereferences
(tests/test_abi_badargs.py's scheme)."""
import ctypes
import functools
import math
from concurrent.futures import ThreadPoolExecutor

import pytest

from dynamicfusion_body_amd import _lib, build

OK, BADARG = 0, -1
PTR = 0x1000                                    # a "device pointer"


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def on_own_thread(test):
    """dfh_last_error() is kept per thread: the refused calls are made on a thread of their own."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        with ThreadPoolExecutor(1) as ex:
            return ex.submit(test, *args, **kwargs).result()
    return run


def problem(**over):
    p = _lib.Problem()
    for f in ("sample_pos", "sample_nrm", "nbr", "weights", "corr", "valid", "node_dq", "node_pos", "node_w", "row_ptr", "col", "vals",
              "rhs", "cost_count", "run_id", "partial", "blk_ptr", "blk_ent", "node_ptr", "node_ent"):
        setattr(p, f, PTR)
    p.n_samples, p.knn, p.n_nodes, p.n_blocks, p.n_rows = 5, 4, 8, 20, 2
    p.lw_dq = (ctypes.c_double * 8)(1.0)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def landmarks(**over):
    t = _lib.Landmarks()
    for f in ("pos", "nbr", "weights", "target", "run_id", "partial", "blk_ptr", "blk_ent", "node_ptr", "node_ent"):
        setattr(t, f, PTR)
    t.n, t.n_rows, t.weight, t.huber_delta, t.max_dist = 7, 3, 1.0, 0.0, 0.0
    for k, v in over.items():
        setattr(t, k, v)
    return t


def solve_params():
    return _lib.SolveParams(pcg_iters=3, x_out=PTR, pcg_workspace=PTR, pcg_workspace_bytes=1 << 30, step=1.0, n_iters=2)


# what a landmark struct is refused for (the table of include/dfusion_hip.h)
BAD_LANDMARKS = {
    "n < 0": dict(n=-1),
    "negative weight": dict(weight=-0.5),
    "infinite weight": dict(weight=math.inf),
    "NaN weight": dict(weight=math.nan),
    "negative huber_delta": dict(huber_delta=-1.0),
    "NaN huber_delta": dict(huber_delta=math.nan),
    "NaN max_dist": dict(max_dist=math.nan),
    "no rows": dict(n_rows=0),
}
BAD_LANDMARKS.update({"null " + f: {f: None} for f in ("pos", "nbr", "weights", "target", "run_id", "partial", "blk_ptr", "blk_ent",
                                                        "node_ptr", "node_ent")})

CALLS = {
    "dfh_gn_add_landmarks": lambda lib, p, t: lib.dfh_gn_add_landmarks(p, t, None),
    "dfh_gn_solve_landmarks": lambda lib, p, t: lib.dfh_gn_solve_landmarks(p, None, t, solve_params(), None),
}


def _refused(lib, name, rc):
    assert rc == BADARG, (name, rc)
    assert name.encode() in lib.dfh_last_error(), (name, lib.dfh_last_error())


@pytest.mark.parametrize("name", sorted(CALLS))
@on_own_thread
def test_landmark_calls_refuse_bad_arguments(lib, name):
    call = CALLS[name]
    _refused(lib, name, call(lib, None, landmarks()))
    _refused(lib, name, call(lib, problem(), None))
    for what, over in BAD_LANDMARKS.items():
        rc = call(lib, problem(), landmarks(**over))
        assert rc == BADARG, (name, what, rc)
        assert name.encode() in lib.dfh_last_error(), (name, what)
    # ... and what the builds refuse of the problem
    _refused(lib, name, call(lib, problem(knn=9), landmarks()))
    _refused(lib, name, call(lib, problem(vals=None), landmarks()))
    _refused(lib, name, call(lib, problem(n_blocks=0), landmarks()))


@on_own_thread
def test_a_term_that_adds_nothing_launches_nothing(lib):
    """n == 0 (null pointers allowed) and weight == 0: DFH_OK without a launch -- there is no GPU here, a launch would fail."""
    nothing = _lib.Landmarks()
    nothing.weight = 1.0
    assert lib.dfh_gn_add_landmarks(problem(), nothing, None) == OK
    assert lib.dfh_gn_add_landmarks(problem(), landmarks(weight=0.0), None) == OK
    assert lib.dfh_gn_add_landmarks(problem(), landmarks(n=0), None) == OK
    # optional pointers: valid, conf and active_out may be null with n > 0 (checked, not launched: weight 0)
    assert lib.dfh_gn_add_landmarks(problem(), landmarks(weight=0.0, valid=None, conf=None, active_out=None), None) == OK


@on_own_thread
def test_solve_landmarks_refuses_what_the_solve_refuses(lib):
    name = "dfh_gn_solve_landmarks"
    _refused(lib, name, lib.dfh_gn_solve_landmarks(problem(blk_ptr=None), None, landmarks(), solve_params(), None))      # no plan
    _refused(lib, name, lib.dfh_gn_solve_landmarks(problem(), None, landmarks(), None, None))                            # no schedule
    sp = solve_params()
    sp.pcg_iters = 0
    _refused(lib, name, lib.dfh_gn_solve_landmarks(problem(), None, landmarks(), sp, None))
    bad_frame = _lib.Frame()                                                                                              # no views
    _refused(lib, name, lib.dfh_gn_solve_landmarks(problem(), bad_frame, landmarks(), solve_params(), None))
    sp = solve_params()
    sp.n_iters = 0                                                                                                        # nothing to do
    assert lib.dfh_gn_solve_landmarks(problem(), None, landmarks(), sp, None) == OK


def test_bindings():
    for name in CALLS:
        assert name in _lib._SIGNATURES and name in _lib.declared_symbols()
    assert _lib.STRUCTS["dfh_gn_landmarks"] is _lib.Landmarks
