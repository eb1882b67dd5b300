"""CPU: what dfh_depth_halve, dfh_icp_track and dfh_icp_track_bytes do with arguments they cannot use.  Validation comes before
any HIP call, so no GPU is needed: device pointers are dummy non-null integers that nothing dereferences
(tests/test_abi_raycast_badargs.py's pattern)."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import pytest

from dynamicfusion_body_amd import _lib, build

OK, BADARG = 0, -1
PTR = 0x1000
INF, NAN = float("inf"), float("nan")


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


def _refused(lib, rc, name):
    assert rc == BADARG, rc
    assert name.encode() in lib.dfh_last_error(), lib.dfh_last_error()


def _params(lib, **over):
    """A call that passes every check (and, with n_iters = 0, launches nothing), then `over` applied to it."""
    eye = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    p = _lib.IcpTrackParams(1, 8, 8, PTR, PTR, PTR, PTR, eye, eye, PTR, 0.1, 0.5, 0.0, 0.0, 0, 6, 1.0, 1.0, PTR, None, PTR,
                            lib.dfh_icp_track_bytes(1))
    k = over.pop("K_entry", None)
    if k is not None:
        p.K[4] = k
    k = over.pop("Kinv_entry", None)
    if k is not None:
        p.Kinv[0] = k
    for name, v in over.items():
        setattr(p, name, v)
    return p


REFUSED = {
    "no views": dict(n_views=0),
    "17 views": dict(n_views=17),
    "H = 0": dict(H=0),
    "W = 0": dict(W=0),
    "H W = 2^31": dict(H=1 << 16, W=1 << 15),
    "null live_depth": dict(live_depth=None),
    "null model_depth": dict(model_depth=None),
    "null model_normals": dict(model_normals=None),
    "null T": dict(T=None),
    "null stats with iterations": dict(stats=None, n_iters=1),
    "null scratch": dict(scratch=None),
    "K nan": dict(K_entry=NAN),
    "Kinv inf": dict(Kinv_entry=INF),
    "max_dist negative": dict(max_dist=-0.1),
    "max_dist nan": dict(max_dist=NAN),
    "max_dist inf": dict(max_dist=INF),
    "min_cos negative": dict(min_cos=-0.1),
    "min_cos above 1": dict(min_cos=1.5),
    "min_cos nan": dict(min_cos=NAN),
    "huber negative": dict(huber=-1.0),
    "huber nan": dict(huber=NAN),
    "lm_rel negative": dict(lm_rel=-1e-3),
    "lm_rel nan": dict(lm_rel=NAN),
    "n_iters -1": dict(n_iters=-1),
    "n_iters 65": dict(n_iters=65),
    "min_count 5": dict(min_count=5),
    "max_rot 0": dict(max_rot=0.0),
    "max_rot nan": dict(max_rot=NAN),
    "max_trans negative": dict(max_trans=-1.0),
    "max_trans nan": dict(max_trans=NAN),
    "scratch too small": dict(scratch_bytes=8),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
@on_own_thread
def test_icp_track_refuses(lib, what):
    _refused(lib, lib.dfh_icp_track(_params(lib, **REFUSED[what]), None), "dfh_icp_track")


@on_own_thread
def test_icp_track_null_params_and_the_call_that_launches_nothing(lib):
    _refused(lib, lib.dfh_icp_track(None, None), "dfh_icp_track")
    assert lib.dfh_icp_track(_params(lib), None) == OK                       # n_iters = 0: checked, nothing launched
    assert lib.dfh_icp_track(_params(lib, stats=None, live_normals=None, max_dist=0.0, max_rot=INF, max_trans=INF), None) == OK


def test_icp_track_bytes(lib):
    assert lib.dfh_icp_track_bytes(0) == 0 and lib.dfh_icp_track_bytes(17) == 0 and lib.dfh_icp_track_bytes(-1) == 0
    one = lib.dfh_icp_track_bytes(1)
    assert one > 0 and one % (29 * 8) == 0
    assert lib.dfh_icp_track_bytes(16) == 16 * one


def _halve(lib, depth=(PTR,), n_views=1, dtype=_lib.F32, H=8, W=8, max_jump=0.1, out=0x2000):
    arr = None if depth is None else (ctypes.c_void_p * len(depth))(*depth)
    return lib.dfh_depth_halve(arr, n_views, dtype, H, W, max_jump, out, None)


HALVE_REFUSED = {
    "null depth array": dict(depth=None),
    "null map": dict(depth=(PTR, None), n_views=2),
    "null out": dict(out=None),
    "out is a map": dict(out=PTR),
    "no views": dict(n_views=0),
    "17 views": dict(depth=(PTR,) * 17, n_views=17),
    "bad dtype": dict(dtype=2),
    "H = 1": dict(H=1),
    "W = 1": dict(W=1),
    "H W = 2^31": dict(H=1 << 16, W=1 << 15),
    "max_jump negative": dict(max_jump=-0.1),
    "max_jump nan": dict(max_jump=NAN),
    "max_jump inf": dict(max_jump=INF),
}


@pytest.mark.parametrize("what", sorted(HALVE_REFUSED))
@on_own_thread
def test_depth_halve_refuses(lib, what):
    _refused(lib, _halve(lib, **HALVE_REFUSED[what]), "dfh_depth_halve")


def test_struct_is_in_the_layout_test():
    """tests/test_abi_symbols.py compares every struct of _lib.STRUCTS with the C compiler's layout: the new one is among them."""
    assert _lib.STRUCTS["dfh_icp_track_params"] is _lib.IcpTrackParams
