"""CPU: what dfh_raycast, dfh_raycast_table and dfh_raycast_table_bytes do with arguments they cannot use.  Validation comes
before any HIP call, so no GPU is needed: device pointers are dummy non-null integers that nothing dereferences
(tests/test_abi_badargs.py's pattern)."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import pytest

from dynamicfusion_body_amd import _lib, build

OK, BADARG = 0, -1
PTR = 0x1000
G = (16, 16, 16)
INF, NAN = float("inf"), float("nan")

BAD_SLABS = {
    "res with a zero": ((4, 0, 4), (0, 4)),
    "x0 > x1": (G, (3, 2)),
    "x1 > res[0]": (G, (0, 17)),
    "65536 planes": ((70000, 4, 4), (0, 65536)),
}


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


def _params(**over):
    """A call that passes every check, then `over` applied to it."""
    keep = []
    slab = over.pop("slab", _lib.slab(G))
    vol = _lib.Volume(PTR, PTR, over.pop("dtype", _lib.F32), slab)
    cslab = over.pop("color_slab", slab)
    cvol = _lib.ColorVolume(over.pop("rgbw", PTR), cslab)
    eye = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    m = (ctypes.c_double * (12 * 16))()
    keep += [vol, cvol, eye, m]
    p = _lib.RaycastParams(ctypes.pointer(vol), None, 1, 8, 8, eye, eye, m, m, 1.0, (ctypes.c_double * 3)(), 8.0, 0.0, INF, 0.5, 0.0, 1, 100,
                           None, 0, PTR, None, None, None)
    if over.pop("with_colors", False):
        p.colors = ctypes.pointer(cvol)
    if over.pop("null_vol", False):
        p.vol = None
    for k, v in over.items():
        setattr(p, k, v)
    p.keep = keep
    return p


def _refused(lib, rc, name="dfh_raycast"):
    assert rc == BADARG, rc
    assert name.encode() in lib.dfh_last_error(), lib.dfh_last_error()


REFUSED = {
    "no volume": dict(null_vol=True),
    "bad dtype": dict(dtype=2),
    "no views": dict(n_views=0),
    "17 views": dict(n_views=17),
    "null lw": dict(lw=None),
    "null wl": dict(wl=None),
    "H = 0": dict(H=0),
    "W = 0": dict(W=0),
    "H W = 2^31": dict(H=1 << 16, W=1 << 15),
    "step 0": dict(step=0.0),
    "step negative": dict(step=-0.5),
    "step inf": dict(step=INF),
    "step nan": dict(step=NAN),
    "z_near negative": dict(z_near=-1.0),
    "z_near inf": dict(z_near=INF),
    "z_near nan": dict(z_near=NAN),
    "z_far == z_near": dict(z_near=1.0, z_far=1.0),
    "z_far nan": dict(z_far=NAN),
    "min_weight negative": dict(min_weight=-1.0),
    "min_weight nan": dict(min_weight=NAN),
    "refine -1": dict(refine=-1),
    "refine 9": dict(refine=9),
    "max_steps 0": dict(max_steps=0),
    "scale 0": dict(scale=0.0),
    "scale inf": dict(scale=INF),
    "scale nan": dict(scale=NAN),
    "no output": dict(depth=None),
    "color without a colour volume": dict(color=PTR),
    "colour volume without rgbw": dict(color=PTR, with_colors=True, rgbw=None),
    "colour volume on another slab": dict(color=PTR, with_colors=True, color_slab=_lib.slab(G, (0, 8))),
    "table too small": dict(table=PTR, table_bytes=7),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
@on_own_thread
def test_raycast_refuses(lib, what):
    _refused(lib, lib.dfh_raycast(_params(**REFUSED[what]), None))


@on_own_thread
def test_raycast_refuses_null_params_and_bad_slabs(lib):
    _refused(lib, lib.dfh_raycast(None, None))
    for res, x_range in BAD_SLABS.values():
        _refused(lib, lib.dfh_raycast(_params(slab=_lib.slab(res, x_range)), None))


@on_own_thread
def test_raycast_table_bytes_and_bad_tables(lib):
    assert lib.dfh_raycast_table_bytes(None) == 0
    for res, x_range in BAD_SLABS.values():
        assert lib.dfh_raycast_table_bytes(_lib.slab(res, x_range)) == 0
    assert lib.dfh_raycast_table_bytes(_lib.slab(G, (2, 2))) == 0
    assert lib.dfh_raycast_table_bytes(_lib.slab(G)) == 8
    assert lib.dfh_raycast_table_bytes(_lib.slab((17, 20, 33))) == 3 * 3 * 5
    assert lib.dfh_raycast_table_bytes(_lib.slab((17, 20, 33), (5, 12))) == 1 * 3 * 5
    assert lib.dfh_raycast_table_bytes(_lib.slab((512, 512, 512))) == 64 ** 3
    name = "dfh_raycast_table"
    _refused(lib, lib.dfh_raycast_table(None, PTR, None), name)
    _refused(lib, lib.dfh_raycast_table(_lib.Volume(PTR, PTR, _lib.F32, _lib.slab(G)), None, None), name)
    _refused(lib, lib.dfh_raycast_table(_lib.Volume(None, PTR, _lib.F32, _lib.slab(G)), PTR, None), name)
    _refused(lib, lib.dfh_raycast_table(_lib.Volume(PTR, PTR, 2, _lib.slab(G)), PTR, None), name)
    for res, x_range in BAD_SLABS.values():
        _refused(lib, lib.dfh_raycast_table(_lib.Volume(PTR, PTR, _lib.F32, _lib.slab(res, x_range)), PTR, None), name)
    assert lib.dfh_raycast_table(_lib.Volume(PTR, PTR, _lib.F32, _lib.slab(G, (2, 2))), PTR, None) == OK     # empty: no launch


def test_raycast_skip_is_an_option(lib):
    _lib.set_option("raycast_skip", 0)
    assert _lib.get_option("raycast_skip") == 0
    _lib.set_option("raycast_skip", None)
    assert _lib.get_option("raycast_skip") == -1


def test_who_builds_a_table():
    """kernels.raycast without a table: option 1 builds one, 0 never, unset only at the sizes where it was measured to pay."""
    from dynamicfusion_body_amd import kernels
    big, many = 256 ** 3, 3 * 640 * 480
    assert kernels.raycast_builds_table(1, 32 ** 3, 64) and not kernels.raycast_builds_table(0, big, many)
    assert kernels.raycast_builds_table(-1, big, many) and kernels.raycast_builds_table(-1, 512 ** 3, 8 * 1280 * 720)
    assert not kernels.raycast_builds_table(-1, big - 1, many) and not kernels.raycast_builds_table(-1, big, 640 * 480 - 1)
