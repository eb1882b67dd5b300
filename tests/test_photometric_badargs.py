"""CPU: what dfh_gn_add_photometric and dfh_gn_solve_photometric do with arguments they cannot use, and with a term that adds nothing.
Validation comes before any HIP call, so no GPU is needed: device pointers are dummy non-null integers that nothing dereferences
(tests/test_landmarks_badargs.py's scheme).  The colour array is a HOST array the checks do read: it is real."""
import ctypes
import functools
import math
from concurrent.futures import ThreadPoolExecutor

import pytest

from dynamicfusion_body_amd import _lib, build

OK, BADARG = 0, -1
PTR = 0x1000                                    # a "device pointer"
N_VIEWS = 3
COLORS = (ctypes.c_void_p * N_VIEWS)(PTR, PTR, PTR)
COLORS_HOLE = (ctypes.c_void_p * N_VIEWS)(PTR, None, PTR)


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


def frame(**over):
    f = _lib.Frame()
    f.views, f.n_views, f.depth_dtype, f.H, f.W, f.scale = PTR, N_VIEWS, _lib.F32, 12, 16, 1.0
    for k, v in over.items():
        setattr(f, k, v)
    return f


def photo(**over):
    t = _lib.Photometric()
    for f in ("pos", "nbr", "weights", "ref", "run_id", "partial", "blk_ptr", "blk_ent", "node_ptr", "node_ent"):
        setattr(t, f, PTR)
    t.color = ctypes.cast(COLORS, ctypes.c_void_p)
    t.n, t.n_rows, t.weight, t.huber_delta, t.max_diff, t.band_sd = 7, 3, 1.0, 0.0, 0.0, 0.5
    for k, v in over.items():
        setattr(t, k, v)
    return t


def solve_params():
    return _lib.SolveParams(pcg_iters=3, x_out=PTR, pcg_workspace=PTR, pcg_workspace_bytes=1 << 30, step=1.0, n_iters=2)


# what a photometric struct is refused for (the table of include/dfusion_hip.h)
BAD_PHOTO = {
    "n < 0": dict(n=-1),
    "negative weight": dict(weight=-0.5),
    "infinite weight": dict(weight=math.inf),
    "NaN weight": dict(weight=math.nan),
    "negative huber_delta": dict(huber_delta=-1.0),
    "NaN huber_delta": dict(huber_delta=math.nan),
    "NaN max_diff": dict(max_diff=math.nan),
    "band_sd 0": dict(band_sd=0.0),
    "negative band_sd": dict(band_sd=-1.0),
    "NaN band_sd": dict(band_sd=math.nan),
    "no rows": dict(n_rows=0),
    "null color": dict(color=None),
    "null color[1]": dict(color=ctypes.cast(COLORS_HOLE, ctypes.c_void_p)),
}
BAD_PHOTO.update({"null " + f: {f: None} for f in ("pos", "nbr", "weights", "ref", "run_id", "partial", "blk_ptr", "blk_ent", "node_ptr",
                                                   "node_ent")})

CALLS = {
    "dfh_gn_add_photometric": lambda lib, p, f, t: lib.dfh_gn_add_photometric(p, f, t, None),
    "dfh_gn_solve_photometric": lambda lib, p, f, t: lib.dfh_gn_solve_photometric(p, f, None, t, solve_params(), None),
}


def _refused(lib, name, rc):
    assert rc == BADARG, (name, rc)
    assert name.encode() in lib.dfh_last_error(), (name, lib.dfh_last_error())


@pytest.mark.parametrize("name", sorted(CALLS))
@on_own_thread
def test_photometric_calls_refuse_bad_arguments(lib, name):
    call = CALLS[name]
    _refused(lib, name, call(lib, None, frame(), photo()))
    _refused(lib, name, call(lib, problem(), None, photo()))                     # a null frame
    if name == "dfh_gn_add_photometric":                                         # (the solve without a term is dfh_gn_solve)
        _refused(lib, name, call(lib, problem(), frame(), None))
    for what, over in BAD_PHOTO.items():
        rc = call(lib, problem(), frame(), photo(**over))
        assert rc == BADARG, (name, what, rc)
        assert name.encode() in lib.dfh_last_error(), (name, what)
    # ... what dfh_gn_associate refuses of the frame
    for over in (dict(views=None), dict(n_views=0), dict(n_views=17), dict(H=1), dict(scale=0.0), dict(depth_dtype=99)):
        _refused(lib, name, call(lib, problem(), frame(**over), photo()))
    # ... and what the builds refuse of the problem
    _refused(lib, name, call(lib, problem(knn=9), frame(), photo()))
    _refused(lib, name, call(lib, problem(vals=None), frame(), photo()))
    _refused(lib, name, call(lib, problem(n_blocks=0), frame(), photo()))
    # the bad settings are refused even when the term would add nothing
    _refused(lib, name, call(lib, problem(), frame(), photo(weight=0.0, band_sd=0.0)))
    _refused(lib, name, call(lib, problem(), frame(), photo(n=0, color=None)))


@on_own_thread
def test_a_term_that_adds_nothing_launches_nothing(lib):
    """n == 0 (null sample pointers allowed) and weight == 0: DFH_OK without a launch -- there is no GPU here, a launch would fail.
    band_sd = +inf is allowed; max_diff and huber_delta may be 0; the optional pointers may be null."""
    nothing = _lib.Photometric()
    nothing.weight, nothing.band_sd, nothing.color = 1.0, 0.5, ctypes.cast(COLORS, ctypes.c_void_p)
    assert lib.dfh_gn_add_photometric(problem(), frame(), nothing, None) == OK
    assert lib.dfh_gn_add_photometric(problem(), frame(), photo(weight=0.0), None) == OK
    assert lib.dfh_gn_add_photometric(problem(), frame(), photo(n=0), None) == OK
    assert lib.dfh_gn_add_photometric(problem(), frame(), photo(weight=0.0, band_sd=math.inf), None) == OK
    assert lib.dfh_gn_add_photometric(problem(), frame(depth_dtype=_lib.F64), photo(weight=0.0), None) == OK     # either depth dtype
    assert lib.dfh_gn_add_photometric(problem(), frame(), photo(weight=0.0, valid=None, conf=None, active_out=None, view_out=None,
                                                                  resid_out=None), None) == OK


@on_own_thread
def test_solve_photometric_refuses_what_the_solve_refuses(lib):
    name = "dfh_gn_solve_photometric"
    call = lambda p, f, l, t, sp: lib.dfh_gn_solve_photometric(p, f, l, t, sp, None)
    _refused(lib, name, call(problem(blk_ptr=None), frame(), None, photo(), solve_params()))          # no plan
    _refused(lib, name, call(problem(), frame(), None, photo(), None))                               # no schedule
    sp = solve_params()
    sp.pcg_iters = 0
    _refused(lib, name, call(problem(), frame(), None, photo(), sp))
    _refused(lib, name, call(problem(), frame(depth_dtype=_lib.F64), None, photo(), solve_params()))   # the fused builds read float32 maps
    bad_lm = _lib.Landmarks()
    bad_lm.n = -1
    _refused(lib, name, call(problem(), frame(), bad_lm, photo(), solve_params()))                   # a landmark term beside it is checked
    sp = solve_params()
    sp.n_iters = 0                                                                                   # nothing to do
    assert call(problem(), frame(), None, photo(), sp) == OK
    # photo == NULL: dfh_gn_solve_landmarks' call (dfh_gn_solve's without landmarks either), which names itself in its refusals
    assert call(problem(), None, None, None, solve_params()) == BADARG and b"dfh_gn_solve:" in lib.dfh_last_error()
    lm = _lib.Landmarks()
    lm.weight = math.nan
    assert call(problem(), None, lm, None, solve_params()) == BADARG and b"dfh_gn_solve_landmarks" in lib.dfh_last_error()
    assert call(problem(), frame(), None, None, sp) == OK and call(problem(), None, _lib.Landmarks(), None, sp) == OK


def test_bindings():
    for name in CALLS:
        assert name in _lib._SIGNATURES and name in _lib.declared_symbols()
    assert _lib.STRUCTS["dfh_gn_photometric"] is _lib.Photometric
