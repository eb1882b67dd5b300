"""CPU: dfh_radius_sample's argument checks (they come before any HIP call: device pointers are dummy non-null integers that
nothing dereferences), its workspace size, and the `sampler` keyword of the three Python layers."""
import ctypes
import functools
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from dynamicfusion_body_amd import Fusion, _lib, build, graph
from dynamicfusion_body_amd.pipeline import SlabFrame

OK, BADARG = 0, -1
PTR = 0x1000                                    # a "device pointer"
NAME = b"dfh_radius_sample"


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


def _call(lib, points=PTR, n=10, radius=1.0, idx=PTR, capacity=10, count="own", rounds="own", ws=PTR, ws_bytes=None):
    cnt, rnd = ctypes.c_long(-7), ctypes.c_int(-7)
    if ws_bytes is None:
        ws_bytes = lib.dfh_radius_sample_workspace_bytes(max(n, 0)) if n < 2 ** 31 else 1 << 40
    rc = lib.dfh_radius_sample(points, n, radius, idx, capacity, ctypes.byref(cnt) if count == "own" else count,
                               ctypes.byref(rnd) if rounds == "own" else rounds, ws, ws_bytes, None)
    return rc, cnt.value, rnd.value


# what is wrong -> keyword arguments of _call
BAD = {
    "n_points < 0": dict(n=-1),
    "n_points = 2^31": dict(n=2 ** 31),
    "n_points = 2^40": dict(n=2 ** 40),
    "radius 0": dict(radius=0.0),
    "radius < 0": dict(radius=-1.0),
    "radius NaN": dict(radius=math.nan),
    "radius inf": dict(radius=math.inf),
    "null points": dict(points=None),
    "null idx_out": dict(idx=None),
    "null count_out": dict(count=None),
    "null workspace": dict(ws=None),
    "capacity < 0": dict(capacity=-1),
    "workspace one byte short": "short",
    "workspace of 0 bytes": dict(ws_bytes=0),
    "bad radius with n_points = 0": dict(n=0, radius=-2.0),
    "null count_out with n_points = 0": dict(n=0, count=None),
}


@pytest.mark.parametrize("what", sorted(BAD))
@on_own_thread
def test_bad_arguments_are_refused_before_any_launch(lib, what):
    kw = BAD[what]
    if kw == "short":
        kw = dict(ws_bytes=lib.dfh_radius_sample_workspace_bytes(10) - 1)
    rc, cnt, _ = _call(lib, **kw)
    assert rc == BADARG, (what, rc)
    assert NAME in lib.dfh_last_error(), (what, lib.dfh_last_error())
    assert cnt == -7                                                    # nothing was written


@on_own_thread
def test_no_points_is_ok_without_a_launch(lib):
    rc, cnt, rnd = _call(lib, n=0, points=None, idx=None, ws=None, ws_bytes=0, capacity=0)
    assert (rc, cnt, rnd) == (OK, 0, 0)
    rc, cnt, _ = _call(lib, n=0, rounds=None)                           # rounds_out may be NULL
    assert (rc, cnt) == (OK, 0)


def test_workspace_bytes_is_monotone_and_small_at_zero(lib):
    f = lib.dfh_radius_sample_workspace_bytes
    assert f(0) <= 4096 and f(-5) == 0
    sizes = [f(n) for n in (1, 2, 255, 256, 257, 1000, 5000, 5001, 10 ** 5, 10 ** 6, 10 ** 7, 2 ** 31 - 1)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    # linear in n beyond the capped cell table: 4 + 1 bytes per point and 8 per 256 points, two tables of 2^21 entries at the most
    assert sizes[-1] <= (2 ** 31) * 5.04 + 2 * 8 * 2 ** 21 + 2 ** 17
    assert f(2 ** 31) == 0                                              # not a valid count


def test_python_layers_refuse_an_unknown_sampler():
    """All three layers check the keyword before they touch the GPU."""
    pts = np.zeros((4, 3))
    with pytest.raises(ValueError, match="sampler"):
        graph.construct_graph_device(pts, 1.0, 4, sampler="bogus")
    with pytest.raises(ValueError, match="sampler"):
        graph.update_graph_device(pts, np.zeros((4, 8)), np.ones(4), pts, 1.0, 4, sampler="bogus")
    fu = Fusion(np.zeros((4, 4, 4)), 1.0, knn=4, write_warpfield=False)
    assert fu.graph_sampler == "host"
    fu._vertices, fu._radius = pts, 1.0
    fu._nodes = [(0, pts[0], graph.NEW_NODE_DQ, 2.0)]
    fu.graph_sampler = "bogus"
    with pytest.raises(ValueError, match="sampler"):
        fu.construct_graph()
    with pytest.raises(ValueError, match="sampler"):
        fu.update_graph(refresh_surface=False)
    sf = SlabFrame.__new__(SlabFrame)                                   # (the constructor allocates volumes on the GPU)
    sf.has_graph = True
    with pytest.raises(ValueError, match="sampler"):
        sf.update_graph(sampler="bogus")
    with pytest.raises(ValueError, match="sampler"):
        sf.construct_graph(2.0, sampler="bogus")
    with pytest.raises(ValueError, match="sampler"):
        sf.step(None, None, update_graph=True, graph_sampler="bogus")
