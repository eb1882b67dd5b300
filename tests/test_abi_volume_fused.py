"""CPU: what the fused entry points of the volume data term -- dfh_gn_build_volume, dfh_gn_solve_volume,
dfh_gn_global_sampled_volume -- do with arguments they cannot use.  Validation comes before any HIP call, so no GPU is needed:
device pointers are dummy non-null integers that nothing dereferences (as in tests/test_associate_volume_cpu.py)."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import pytest

from dynamicfusion_body_amd import _lib, build

OK, BADARG = 0, -1
PTR = 0x1000                                    # a "device pointer"
NAN, INF = float("nan"), float("inf")
BIG = 1 << 30                                   # a scratch size that is always enough


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
    """A planned problem with every pointer set."""
    p = _lib.Problem()
    for f, t in _lib.Problem._fields_:
        if t is ctypes.c_void_p:
            setattr(p, f, PTR)
    p.n_samples, p.knn, p.n_nodes, p.n_blocks, p.n_upper, p.n_rows = 5, 4, 8, 8, 0, 2
    p.lw_dq = (ctypes.c_double * 8)(1.0)
    p.rw, p.huber_delta = 0.0, 0.0
    for k, v in over.items():
        setattr(p, k, v)
    return p


def term(data=PTR, dtype=_lib.F32, res=(4, 4, 4), value_to_vox=1.0, band=4.0, max_dist=0.0, min_grad=0.5):
    return _lib.VolumeTerm(_lib.Live(data, dtype, _lib.iarr(res)), value_to_vox, band, max_dist, min_grad)


def params(**over):
    sp = _lib.SolveParams()
    sp.pcg_iters, sp.lm_abs, sp.lm_rel, sp.step = 10, 0.0, 0.0, 1.0
    sp.x_out, sp.pcg_workspace, sp.pcg_workspace_bytes = PTR, PTR, BIG
    sp.n_iters, sp.n_global, sp.global_lm = 1, 0, 0.1
    sp.global_scratch, sp.global_scratch_bytes = PTR, BIG
    for k, v in over.items():
        setattr(sp, k, v)
    return sp


CALLS = {
    "dfh_gn_build_volume": lambda lib, p, t, sp=None, **kw: lib.dfh_gn_build_volume(p, t, None),
    "dfh_gn_solve_volume": lambda lib, p, t, sp=None, **kw: lib.dfh_gn_solve_volume(p, t, params() if sp is None else sp, None),
    "dfh_gn_global_sampled_volume": lambda lib, p, t, sp=None, stride=1, n_steps=1, sums=0, scratch=PTR, nbytes=BIG, **kw:
        lib.dfh_gn_global_sampled_volume(p, t, stride, 0.1, n_steps, PTR, sums, scratch, nbytes, None),
}
FUSED = ("dfh_gn_build_volume", "dfh_gn_solve_volume")

# what all three refuse: (problem, term)
BAD = {
    "null problem": lambda: (None, term()),
    "null term": lambda: (problem(), None),
    "null live.data": lambda: (problem(), term(data=0)),
    "dtype 2": lambda: (problem(), term(dtype=2)),
    "res[0] 1": lambda: (problem(), term(res=(1, 4, 4))),
    "res[1] 1": lambda: (problem(), term(res=(4, 1, 4))),
    "res[2] 0": lambda: (problem(), term(res=(4, 4, 0))),
    "band 0": lambda: (problem(), term(band=0.0)),
    "band -1": lambda: (problem(), term(band=-1.0)),
    "band nan": lambda: (problem(), term(band=NAN)),
    "min_grad nan": lambda: (problem(), term(min_grad=NAN)),
    "min_grad -1": lambda: (problem(), term(min_grad=-1.0)),
    "max_dist nan": lambda: (problem(), term(max_dist=NAN)),
    "value_to_vox 0": lambda: (problem(), term(value_to_vox=0.0)),
    "value_to_vox inf": lambda: (problem(), term(value_to_vox=INF)),
    "value_to_vox nan": lambda: (problem(), term(value_to_vox=NAN)),
    "knn 9": lambda: (problem(knn=9), term()),
    "null node_dq": lambda: (problem(node_dq=0), term()),
    "null sample_nrm": lambda: (problem(sample_nrm=0), term()),
}


def _refused(lib, name, rc, case):
    assert rc == BADARG, (name, case, rc)
    assert name.encode() in lib.dfh_last_error(), (name, case, lib.dfh_last_error())


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("name", sorted(CALLS))
@on_own_thread
def test_bad_problems_and_terms_are_refused(lib, name, case):
    p, t = BAD[case]()
    _refused(lib, name, CALLS[name](lib, p, t), case)


@pytest.mark.parametrize("name", FUSED)
@on_own_thread
def test_fused_calls_need_a_plan_and_a_float32_volume(lib, name):
    _refused(lib, name, CALLS[name](lib, problem(), term(dtype=_lib.F64)), "float64 live volume")
    _refused(lib, name, CALLS[name](lib, problem(blk_ptr=0), term()), "no plan")
    _refused(lib, name, CALLS[name](lib, problem(vals=0), term()), "no system")


@on_own_thread
def test_solve_volume_refuses_bad_schedules(lib):
    name = "dfh_gn_solve_volume"
    assert lib.dfh_gn_solve_volume(problem(), term(), None, None) == BADARG
    assert name.encode() in lib.dfh_last_error()
    for case, sp in (("n_iters 1001", params(n_iters=1001)), ("n_iters -1", params(n_iters=-1)), ("n_global 101", params(n_global=101)),
                     ("n_global -1", params(n_global=-1)), ("pcg_iters 0", params(pcg_iters=0)), ("null x_out", params(x_out=0)),
                     ("null workspace", params(pcg_workspace=0))):
        _refused(lib, name, CALLS[name](lib, problem(), term(), sp=sp), case)


@on_own_thread
def test_sampled_volume_step_refuses_bad_schedules(lib):
    name = "dfh_gn_global_sampled_volume"
    call = CALLS[name]
    _refused(lib, name, call(lib, problem(), term(), stride=0), "stride 0")
    _refused(lib, name, call(lib, problem(), term(), n_steps=101), "n_steps 101")
    _refused(lib, name, call(lib, problem(), term(), n_steps=-1), "n_steps -1")
    need = lib.dfh_gn_global_sampled_bytes(5, 1)
    assert need > 0
    _refused(lib, name, call(lib, problem(), term(), nbytes=need - 1), "scratch too small")
    _refused(lib, name, call(lib, problem(), term(), scratch=0), "null scratch")
    _refused(lib, name, call(lib, problem(), term(), sums=PTR, n_steps=2), "sums_out with two steps")
    # no step: nothing to check, nothing to launch -- also with a term that would be refused, a float64 volume, no plan
    assert call(lib, problem(), term(), n_steps=0) == OK
    assert call(lib, problem(blk_ptr=0), term(dtype=_lib.F64, band=0.0), n_steps=0) == OK
    # ... but the step count and the stride are checked first
    _refused(lib, name, call(lib, problem(), term(), n_steps=0, stride=0), "stride 0 without steps")


def test_the_abi_version_did_not_move(lib):
    assert lib.dfh_version() == 8 == _lib.ABI_VERSION
    for name in CALLS:
        assert name in _lib._SIGNATURES and name in _lib.declared_symbols()
