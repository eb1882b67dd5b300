"""CPU: what the K23 entry points (dfh_mesh_components, dfh_mesh_component_table, dfh_mesh_compact and their size query) do with
arguments they cannot use.  Validation comes before any HIP call, so no GPU is needed: the device pointers are dummy non-null
integers that nothing dereferences (tests/test_abi_mesh_sdf_badargs.py's pattern)."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from dynamicfusion_body_amd import _lib, build, mesh

OK, BADARG = 0, -1
PTR = 0x1000
V, F, C = 10, 6, 3


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


def _label(lib, **over):
    a = dict(faces=PTR, V=V, F=F, root=PTR, vert_comp=PTR, face_comp=PTR, n=ctypes.c_long(-7), ws=PTR, ws_bytes=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = lib.dfh_mesh_components_workspace_bytes(V, F)
    n = a["n"]
    return lib.dfh_mesh_components(a["faces"], a["V"], a["F"], a["root"], a["vert_comp"], a["face_comp"], None if n is None else ctypes.byref(n),
                                   a["ws"], a["ws_bytes"], None)


def _table(lib, **over):
    a = dict(verts=PTR, dtype=_lib.F64, V=V, faces=PTR, F=F, root=PTR, vert_comp=PTR, face_comp=PTR, C=C, comp_root=PTR, n_verts=PTR,
             n_faces=PTR, bbox_min=PTR, bbox_max=PTR, area=PTR, ws=PTR, ws_bytes=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = lib.dfh_mesh_components_workspace_bytes(V, F)
    return lib.dfh_mesh_component_table(a["verts"], a["dtype"], a["V"], a["faces"], a["F"], a["root"], a["vert_comp"], a["face_comp"], a["C"],
                                        a["comp_root"], a["n_verts"], a["n_faces"], a["bbox_min"], a["bbox_max"], a["area"], a["ws"],
                                        a["ws_bytes"], None)


def _compact(lib, **over):
    a = dict(faces=PTR, V=V, F=F, vert_comp=PTR, face_comp=PTR, keep=PTR, C=C, drop=1, kept=PTR, vmap=PTR, fout=PTR,
             counts=(ctypes.c_long * 2)(-7, -7), ws=PTR, ws_bytes=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = lib.dfh_mesh_components_workspace_bytes(V, F)
    return lib.dfh_mesh_compact(a["faces"], a["V"], a["F"], a["vert_comp"], a["face_comp"], a["keep"], a["C"], a["drop"], a["kept"], a["vmap"],
                                a["fout"], a["counts"], a["ws"], a["ws_bytes"], None)


SIZES = {
    "V negative": dict(V=-1),
    "V = 2^31": dict(V=1 << 31),
    "F negative": dict(F=-1),
    "F = 2^31": dict(F=1 << 31),
}
WORKSPACE = {
    "null workspace": dict(ws=None),
    "misaligned workspace": dict(ws=PTR + 4),
    "workspace one byte short": dict(ws_bytes=-1),          # (resolved below)
    "workspace of nothing": dict(ws_bytes=0),
}
LABEL_REFUSED = dict(SIZES, **WORKSPACE, **{
    "null faces": dict(faces=None),
    "null face_comp": dict(face_comp=None),
    "null root": dict(root=None),
    "null vert_comp": dict(vert_comp=None),
    "null n_components": dict(n=None),
})
TABLE_REFUSED = dict(SIZES, **WORKSPACE, **{
    "null verts": dict(verts=None),
    "null faces": dict(faces=None),
    "null root": dict(root=None),
    "null vert_comp": dict(vert_comp=None),
    "null face_comp": dict(face_comp=None),
    "unknown dtype": dict(dtype=2),
    "negative dtype": dict(dtype=-1),
    "C negative": dict(C=-1),
    "C above V": dict(C=V + 1),
    "null comp_root": dict(comp_root=None),
    "null n_verts": dict(n_verts=None),
    "null n_faces": dict(n_faces=None),
    "null bbox_min": dict(bbox_min=None),
    "null bbox_max": dict(bbox_max=None),
    "null area": dict(area=None),
})
COMPACT_REFUSED = dict(SIZES, **WORKSPACE, **{
    "null faces": dict(faces=None),
    "null vert_comp": dict(vert_comp=None),
    "null face_comp": dict(face_comp=None),
    "null keep": dict(keep=None),
    "C negative": dict(C=-1),
    "C above V": dict(C=V + 1),
    "drop_unreferenced 2": dict(drop=2),
    "drop_unreferenced -1": dict(drop=-1),
    "null kept_vert_idx": dict(kept=None),
    "null vert_map": dict(vmap=None),
    "null faces_out": dict(fout=None),
    "null counts_out": dict(counts=None),
})


def _resolve(lib, over):
    over = dict(over)
    if over.get("ws_bytes") == -1:
        over["ws_bytes"] = lib.dfh_mesh_components_workspace_bytes(V, F) - 1
    return over


@pytest.mark.parametrize("what", sorted(LABEL_REFUSED))
@on_own_thread
def test_components_refuses(lib, what):
    n = ctypes.c_long(-7)
    over = _resolve(lib, LABEL_REFUSED[what])
    over.setdefault("n", n)
    _refused(lib, _label(lib, **over), "dfh_mesh_components")
    assert n.value == -7                                    # nothing was written


@pytest.mark.parametrize("what", sorted(TABLE_REFUSED))
@on_own_thread
def test_table_refuses(lib, what):
    _refused(lib, _table(lib, **_resolve(lib, TABLE_REFUSED[what])), "dfh_mesh_component_table")


@pytest.mark.parametrize("what", sorted(COMPACT_REFUSED))
@on_own_thread
def test_compact_refuses(lib, what):
    counts = (ctypes.c_long * 2)(-7, -7)
    over = _resolve(lib, COMPACT_REFUSED[what])
    over.setdefault("counts", counts)
    _refused(lib, _compact(lib, **over), "dfh_mesh_compact")
    assert list(counts) == [-7, -7]                          # nothing was written


@on_own_thread
def test_empty_meshes_are_valid_and_launch_nothing(lib):
    n = ctypes.c_long(-7)
    assert _label(lib, V=0, F=0, faces=None, root=None, vert_comp=None, face_comp=None, n=n, ws=None, ws_bytes=0) == OK and n.value == 0
    assert _table(lib, V=0, F=0, C=0, verts=None, faces=None, root=None, vert_comp=None, face_comp=None, comp_root=None, n_verts=None,
                  n_faces=None, bbox_min=None, bbox_max=None, area=None, ws=None, ws_bytes=0) == OK
    counts = (ctypes.c_long * 2)(-7, -7)
    assert _compact(lib, V=0, F=0, C=0, faces=None, vert_comp=None, face_comp=None, keep=None, kept=None, vmap=None, fout=None, counts=counts,
                    ws=None, ws_bytes=0) == OK
    assert list(counts) == [0, 0]


def test_workspace_size(lib):
    size = lib.dfh_mesh_components_workspace_bytes
    assert size(-1, 0) == 0 and size(0, -1) == 0 and size(1 << 31, 0) == 0 and size(0, 1 << 31) == 0
    assert size(0, 0) > 0 and size(0, 0) % 8 == 0
    assert size(1000, 2000) % 8 == 0 and size(1000, 2000) > size(1000, 1000) > size(10, 10)
    assert size(800_000, 1_500_000) < 64 << 20              # the 512^3 scene mesh: tens of megabytes


PY_REFUSED = {
    "verts (V, 2)": (np.zeros((4, 2)), np.zeros((1, 3), dtype=np.int32)),
    "verts int": (np.zeros((4, 3), dtype=np.int64), np.zeros((1, 3), dtype=np.int32)),
    "faces (F, 4)": (np.zeros((4, 3)), np.zeros((1, 4), dtype=np.int32)),
    "faces float": (np.zeros((4, 3)), np.zeros((1, 3))),
}


@pytest.mark.parametrize("what", sorted(PY_REFUSED))
def test_python_refuses_before_it_needs_a_gpu(lib, what):
    with pytest.raises(ValueError):
        mesh.connected_components(*PY_REFUSED[what])


def test_the_new_entry_points_are_bound():
    for name in ("dfh_mesh_components_workspace_bytes", "dfh_mesh_components", "dfh_mesh_component_table", "dfh_mesh_compact"):
        assert name in _lib._SIGNATURES and name in _lib.declared_symbols()
    assert _lib.ABI_VERSION == 8
