"""CPU: what the dfh_mesh_sdf_* entry points do with arguments they cannot use.  Validation comes before any device work, so no
GPU is needed: dfh_mesh_sdf_plan reads host arrays only, and the device pointers given to the others are dummy non-null
integers that nothing dereferences (tests/test_abi_raycast_badargs.py's pattern)."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from dynamicfusion_body_amd import _lib, build, mesh

OK, BADARG = 0, -1
PTR = 0x1000
INF, NAN = float("inf"), float("nan")

V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)
KEEP = np.ones(4, dtype=np.uint8)


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


def _plan(lib, v=V, f=F, keep=KEEP, cell=0.0, nv=None, nf=None, out=True):
    lay = _lib.MeshSdfLayout()
    rc = lib.dfh_mesh_sdf_plan(None if v is None else v.ctypes.data, len(V) if nv is None else nv, None if f is None else f.ctypes.data,
                               None if keep is None else keep.ctypes.data, len(F) if nf is None else nf, cell, lay if out else None)
    return rc, lay


def _with(a, index, value):
    b = a.copy()
    b[index] = value
    return b


PLAN_REFUSED = {
    "null verts": dict(v=None),
    "null faces": dict(f=None),
    "null keep": dict(keep=None),
    "null layout": dict(out=False),
    "F == 0": dict(nf=0),
    "no vertices": dict(nv=0),
    "index == n_verts": dict(f=_with(F, (3, 2), 4)),
    "index negative": dict(f=_with(F, (0, 0), -1)),
    "vertex nan": dict(v=_with(V, (2, 1), NAN)),
    "vertex inf": dict(v=_with(V, (0, 0), INF)),
    "nothing kept": dict(keep=np.zeros(4, dtype=np.uint8)),
    "cell negative": dict(cell=-1.0),
    "cell nan": dict(cell=NAN),
    "cell inf": dict(cell=INF),
}


@pytest.mark.parametrize("what", sorted(PLAN_REFUSED))
@on_own_thread
def test_plan_refuses(lib, what):
    _refused(lib, _plan(lib, **PLAN_REFUSED[what])[0], "dfh_mesh_sdf_plan")


@on_own_thread
def test_plan_lays_the_table_out(lib):
    rc, lay = _plan(lib)
    assert rc == OK, lib.dfh_last_error()
    assert list(lay.lo) == [0, 0, 0] and list(lay.hi) == [1, 1, 1] and lay.maxabs == 1.0
    assert lay.cell == 2.0 and list(lay.dims) == [1, 1, 1] and lay.n_entries == 4                # twice the mean face extent
    assert lay.bytes == 8 + 8 + 4 * 8 + 4 * 8
    rc, lay = _plan(lib, cell=0.5)
    assert rc == OK and lay.cell == 0.5 and list(lay.dims) == [3, 3, 3]
    assert lay.n_entries == 3 * 9 + 27                      # three axis-aligned faces in a 3 x 3 x 1 slab each, the slanted one everywhere
    rc, lay = _plan(lib, cell=1e-9)
    assert rc == OK and lay.cell == 1.0 / 127 and 127 <= max(lay.dims) <= 128                           # never more than 128 cells an axis
    assert lib.dfh_mesh_sdf_chunk() == 64


def _mesh(lib, **over):
    lay = over.pop("layout", None) or _plan(lib)[1]
    m = _lib.MeshSdf(PTR, PTR, PTR, PTR, PTR, PTR, len(V), len(F), PTR, lay.bytes, lay)
    for k, v in over.items():
        setattr(m, k, v)
    return m


def _bad_layout(lib, **over):
    lay = _plan(lib)[1]
    for k, v in over.items():
        setattr(lay, k, v)
    return lay


def bad_meshes(lib):
    yield None
    for field in ("verts", "faces", "keep", "face_normals", "edge_normals", "vertex_normals", "table"):
        yield _mesh(lib, **{field: None})
    yield _mesh(lib, n_faces=5)
    yield _mesh(lib, n_verts=3)
    yield _mesh(lib, table_bytes=_plan(lib)[1].bytes - 1)
    yield _mesh(lib, layout=_bad_layout(lib, cell=0.0))
    yield _mesh(lib, layout=_bad_layout(lib, cell=NAN))
    yield _mesh(lib, layout=_bad_layout(lib, dims=_lib.iarr((1, 129, 1))))
    yield _mesh(lib, layout=_bad_layout(lib, n_entries=0))
    yield _mesh(lib, layout=_bad_layout(lib, n_entries=5))                                      # bytes no longer match
    yield _mesh(lib, layout=_bad_layout(lib, lo=(ctypes.c_double * 3)(2, 0, 0)))


def _grid(**over):
    g = _lib.MeshSdfGridParams((ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(1, 1, 1), _lib.iarr((4, 4, 4)), 2.0, 1, _lib.F32,
                               PTR, PTR, None, None)
    for k, v in over.items():
        setattr(g, k, v)
    return g


@on_own_thread
def test_build_and_queries_refuse_bad_meshes(lib):
    pts = lambda m: lib.dfh_mesh_sdf_points(m, PTR, 10, INF, 1, PTR, PTR, PTR, None)
    for m in bad_meshes(lib):
        _refused(lib, lib.dfh_mesh_sdf_build(m, None), "dfh_mesh_sdf_build")
        _refused(lib, pts(m), "dfh_mesh_sdf_points")
        _refused(lib, lib.dfh_mesh_sdf_grid(m, _grid(), None), "dfh_mesh_sdf_grid")


POINTS_REFUSED = {
    "null points": dict(points=None),
    "null sdist": dict(sdist=None),
    "n negative": dict(n=-1),
    "n = 2^31": dict(n=1 << 31),
    "band 0": dict(band=0.0),
    "band negative": dict(band=-1.0),
    "band nan": dict(band=NAN),
    "orientation 0": dict(orientation=0),
    "orientation 2": dict(orientation=2),
}


@pytest.mark.parametrize("what", sorted(POINTS_REFUSED))
@on_own_thread
def test_points_refuses(lib, what):
    a = dict(points=PTR, n=10, band=INF, orientation=1, sdist=PTR)
    a.update(POINTS_REFUSED[what])
    _refused(lib, lib.dfh_mesh_sdf_points(_mesh(lib), a["points"], a["n"], a["band"], a["orientation"], a["sdist"], None, None, None),
             "dfh_mesh_sdf_points")


@on_own_thread
def test_points_with_no_point_is_ok(lib):
    assert lib.dfh_mesh_sdf_points(_mesh(lib), None, 0, INF, 1, None, None, None, None) == OK      # nothing launched


GRID_REFUSED = {
    "null value": dict(value=None),
    "bad dtype": dict(dtype=2),
    "band 0": dict(band=0.0),
    "band negative": dict(band=-2.0),
    "band nan": dict(band=NAN),
    "orientation 0": dict(orientation=0),
    "shape with a zero": dict(shape=_lib.iarr((4, 0, 4))),
    "2^31 vertices": dict(shape=_lib.iarr((2048, 1024, 1024))),
    "origin nan": dict(origin=(ctypes.c_double * 3)(0, NAN, 0)),
    "origin inf": dict(origin=(ctypes.c_double * 3)(INF, 0, 0)),
    "spacing 0": dict(spacing=(ctypes.c_double * 3)(1, 0, 1)),
    "spacing negative": dict(spacing=(ctypes.c_double * 3)(1, 1, -1)),
    "spacing nan": dict(spacing=(ctypes.c_double * 3)(NAN, 1, 1)),
    "spacing inf": dict(spacing=(ctypes.c_double * 3)(1, INF, 1)),
    "band below max(spacing)": dict(spacing=(ctypes.c_double * 3)(1, 2.5, 1)),
    "finite band without status": dict(status=None),
}


@pytest.mark.parametrize("what", sorted(GRID_REFUSED))
@on_own_thread
def test_grid_refuses(lib, what):
    _refused(lib, lib.dfh_mesh_sdf_grid(_mesh(lib), _grid(**GRID_REFUSED[what]), None), "dfh_mesh_sdf_grid")


@on_own_thread
def test_grid_refuses_null_params(lib):
    _refused(lib, lib.dfh_mesh_sdf_grid(_mesh(lib), None, None), "dfh_mesh_sdf_grid")


PY_REFUSED = {
    "F == 0": (V, np.zeros((0, 3), dtype=np.int32), {}),
    "index out of range": (V, _with(F, (1, 1), 4), {}),
    "vertex nan": (_with(V, (1, 1), NAN), F, {}),
    "all faces zero-area": (V, np.array([[0, 0, 1], [2, 2, 2]]), {}),
    "float faces": (V, F.astype(np.float64), {}),
    "verts (N, 2)": (V[:, :2], F, {}),
    "orientation 0": (V, F, dict(orientation=0)),
    "cell 0": (V, F, dict(cell=0.0)),
    "cell nan": (V, F, dict(cell=NAN)),
}


@pytest.mark.parametrize("what", sorted(PY_REFUSED))
@on_own_thread
def test_python_refuses_before_it_needs_a_gpu(lib, what):
    v, f, kw = PY_REFUSED[what]
    with pytest.raises(ValueError):
        mesh.MeshDistance(v, f, **kw)


def test_the_new_entry_points_and_structs_are_bound():
    for name in ("dfh_mesh_sdf_chunk", "dfh_mesh_sdf_plan", "dfh_mesh_sdf_build", "dfh_mesh_sdf_points", "dfh_mesh_sdf_grid"):
        assert name in _lib._SIGNATURES and name in _lib.declared_symbols()
    assert _lib.STRUCTS["dfh_mesh_sdf"] is _lib.MeshSdf and _lib.STRUCTS["dfh_mesh_sdf_layout"] is _lib.MeshSdfLayout
    assert _lib.STRUCTS["dfh_mesh_sdf_grid_params"] is _lib.MeshSdfGridParams
    assert _lib.ABI_VERSION == 8
