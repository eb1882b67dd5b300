"""CPU: what the K25 entry points (dfh_mesh_smooth_prepare, _run, dfh_mesh_vertex_normals and their size query) do with arguments
they cannot use.  Validation comes before any HIP call, so no GPU is needed: the device pointers are dummy non-null integers
that nothing dereferences (tests/test_abi_simplify_badargs.py's pattern)."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from dynamicfusion_body_amd import _lib, build, mesh

OK, BADARG = 0, -1
PTR = 0x1000
V, F = 10, 6
NAN, INF = float("nan"), float("inf")
NAMES = ("dfh_mesh_smooth_workspace_bytes", "dfh_mesh_smooth_prepare", "dfh_mesh_smooth_run", "dfh_mesh_vertex_normals")


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


def _ws_bytes(lib, a):
    if a["ws_bytes"] is None:
        return lib.dfh_mesh_smooth_workspace_bytes(max(a["V"], 0), max(a["F"], 0)) or lib.dfh_mesh_smooth_workspace_bytes(V, F)
    if a["ws_bytes"] == -1:
        return lib.dfh_mesh_smooth_workspace_bytes(V, F) - 1
    return a["ws_bytes"]


def _prepare(lib, **over):
    a = dict(verts=PTR, dtype=_lib.F64, V=V, faces=PTR, F=F, scv=PTR, corder=PTR, weights=0, bnd=PTR, ws=PTR, ws_bytes=None)
    a.update(over)
    return lib.dfh_mesh_smooth_prepare(a["verts"], a["dtype"], a["V"], a["faces"], a["F"], a["scv"], a["corder"], a["weights"], a["bnd"], a["ws"],
                                       _ws_bytes(lib, a), None)


def _run(lib, **over):
    a = dict(x=PTR, dtype=_lib.F32, V=V, F=F, K=3, weights=0, boundary=0, layout=0, iters=2, lam=0.5, mu=-0.53, out=PTR, ws=PTR, ws_bytes=None)
    a.update(over)
    return lib.dfh_mesh_smooth_run(a["x"], a["dtype"], a["V"], a["F"], a["K"], a["weights"], a["boundary"], a["layout"], a["iters"], a["lam"], a["mu"],
                                   a["out"], a["ws"], _ws_bytes(lib, a), None)


def _normals(lib, **over):
    a = dict(verts=PTR, dtype=_lib.F32, V=V, F=F, sign=-1.0, out=PTR, ws=PTR, ws_bytes=None)
    a.update(over)
    return lib.dfh_mesh_vertex_normals(a["verts"], a["dtype"], a["V"], a["F"], a["sign"], a["out"], a["ws"], _ws_bytes(lib, a), None)


SIZES = {
    "V negative": dict(V=-1),
    "V = 2^31": dict(V=1 << 31),
    "F negative": dict(F=-1),
    "3F beyond an int": dict(F=((1 << 31) - 1) // 3 + 1),
    "faces without vertices": dict(V=0),
    "unknown dtype": dict(dtype=2),
    "negative dtype": dict(dtype=-1),
}
WORKSPACE = {
    "null workspace": dict(ws=None),
    "misaligned workspace": dict(ws=PTR + 8),
    "workspace one byte short": dict(ws_bytes=-1),
    "workspace of nothing": dict(ws_bytes=0),
}
PREPARE_REFUSED = dict(SIZES, **WORKSPACE, **{
    "unknown weights": dict(weights=2),
    "negative weights": dict(weights=-1),
    "null verts": dict(verts=None),
    "null faces": dict(faces=None),
    "null sorted_corner_vert": dict(scv=None),
    "null corner_order": dict(corder=None),
})
RUN_REFUSED = dict(SIZES, **WORKSPACE, **{
    "width 0": dict(K=0),
    "width 5": dict(K=5),
    "width negative": dict(K=-1),
    "unknown weights": dict(weights=2),
    "unknown boundary": dict(boundary=2),
    "negative boundary": dict(boundary=-1),
    "unknown layout": dict(layout=2),
    "iters negative": dict(iters=-1),
    "lam NaN": dict(lam=NAN),
    "lam infinite": dict(lam=INF),
    "mu NaN": dict(mu=NAN),
    "mu infinite": dict(mu=-INF),
    "null x": dict(x=None),
    "null out": dict(out=None),
})
NORMALS_REFUSED = dict(SIZES, **WORKSPACE, **{
    "sign NaN": dict(sign=NAN),
    "sign infinite": dict(sign=INF),
    "null verts": dict(verts=None),
    "null normals": dict(out=None),
})


@pytest.mark.parametrize("what", sorted(PREPARE_REFUSED))
@on_own_thread
def test_prepare_refuses(lib, what):
    _refused(lib, _prepare(lib, **PREPARE_REFUSED[what]), "dfh_mesh_smooth_prepare")


@pytest.mark.parametrize("what", sorted(RUN_REFUSED))
@on_own_thread
def test_run_refuses(lib, what):
    _refused(lib, _run(lib, **RUN_REFUSED[what]), "dfh_mesh_smooth_run")


@pytest.mark.parametrize("what", sorted(NORMALS_REFUSED))
@on_own_thread
def test_vertex_normals_refuses(lib, what):
    _refused(lib, _normals(lib, **NORMALS_REFUSED[what]), "dfh_mesh_vertex_normals")


@on_own_thread
def test_empty_meshes_are_valid_and_launch_nothing(lib):
    assert _prepare(lib, V=0, F=0, verts=None, faces=None, scv=None, corder=None, bnd=None, ws=None, ws_bytes=0) == OK
    assert _run(lib, V=0, F=0, x=None, out=None, ws=None, ws_bytes=0) == OK
    assert _normals(lib, V=0, F=0, verts=None, out=None, ws=None, ws_bytes=0) == OK


def test_workspace_size(lib):
    size = lib.dfh_mesh_smooth_workspace_bytes
    assert size(-1, 0) == 0 and size(0, -1) == 0 and size(1 << 31, 0) == 0 and size(0, ((1 << 31) - 1) // 3 + 1) == 0
    assert size(0, 0) > 0 and size(0, 0) % 32 == 0
    assert size(1000, 2000) % 32 == 0 and size(1000, 2000) > size(1000, 1000) > size(10, 10)
    assert size(2000, 1000) > size(1000, 1000)
    last = 0
    for n in (0, 1, 7, 1023, 1024, 1025, 4096, 100_000):     # monotone in both counts
        assert size(n, n) > last and size(n + 1, n) >= size(n, n) and size(n, n + 1) >= size(n, n)
        last = size(n, n)
    # 72 bytes a face (neighbour and weight pairs of its three entries), 73 a vertex (two rows of four doubles, the bounds, the flag)
    assert size(800_000, 1_570_000) < 176 << 20             # the 512^3 scene mesh


PY_REFUSED = {
    "verts (V, 2)": (dict(), np.zeros((4, 2)), np.zeros((1, 3), dtype=np.int32)),
    "verts int": (dict(), np.zeros((4, 3), dtype=np.int64), np.zeros((1, 3), dtype=np.int32)),
    "faces (F, 4)": (dict(), np.zeros((4, 3)), np.zeros((1, 4), dtype=np.int32)),
    "faces float": (dict(), np.zeros((4, 3)), np.zeros((1, 3))),
    "unknown weights": (dict(weights="mean-value"), np.zeros((4, 3)), np.zeros((1, 3), dtype=np.int32)),
    "unknown boundary": (dict(boundary="pinned"), np.zeros((4, 3)), np.zeros((1, 3), dtype=np.int32)),
}


@pytest.mark.parametrize("what", sorted(PY_REFUSED))
def test_python_refuses_before_it_needs_a_gpu(lib, what):
    kw, *args = PY_REFUSED[what]
    with pytest.raises(ValueError):
        mesh.smooth(*args, **kw)
    with pytest.raises(ValueError):
        mesh.MeshLaplacian(*args, **kw)


def test_taubin_mu_is_the_pass_band_formula_in_fp64():
    assert mesh.taubin_mu(0.5, 0.1) == 1.0 / (0.1 - 1.0 / 0.5)
    for lam, pb in ((0.0, 0.1), (NAN, 0.1), (0.5, NAN), (0.5, 2.0)):
        with pytest.raises(ValueError):
            mesh.taubin_mu(lam, pb)


def test_the_new_entry_points_are_bound(lib):
    for name in NAMES:
        assert name in _lib._SIGNATURES and name in _lib.declared_symbols() and hasattr(lib, name)
    assert _lib.ABI_VERSION == 8 and lib.dfh_version() == 8
