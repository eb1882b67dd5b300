"""CPU: what the K24 entry points (dfh_mesh_simplify_keys, _group, _clusters, _attr, _faces and their size query) do with arguments
they cannot use.  Validation comes before any HIP call, so no GPU is needed: the device pointers are dummy non-null integers
that nothing dereferences (tests/test_abi_components_badargs.py's pattern)."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from dynamicfusion_body_amd import _lib, build, mesh

OK, BADARG = 0, -1
PTR = 0x1000
V, F, C, K = 10, 6, 3, 4
NAN, INF = float("nan"), float("inf")
NAMES = ("dfh_mesh_simplify_workspace_bytes", "dfh_mesh_simplify_keys", "dfh_mesh_simplify_group", "dfh_mesh_simplify_clusters",
         "dfh_mesh_simplify_attr", "dfh_mesh_simplify_faces")


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


def _origin(o):
    return None if o is None else (ctypes.c_double * 3)(*o)


def _ws_bytes(lib, a):
    if a["ws_bytes"] is None:
        return lib.dfh_mesh_simplify_workspace_bytes(V, F)
    if a["ws_bytes"] == -1:
        return lib.dfh_mesh_simplify_workspace_bytes(V, F) - 1
    return a["ws_bytes"]


def _keys(lib, **over):
    a = dict(verts=PTR, dtype=_lib.F64, V=V, faces=PTR, F=F, cell=1.0, origin=(0.0, 0.0, 0.0), keys=PTR, ws=PTR, ws_bytes=None)
    a.update(over)
    return lib.dfh_mesh_simplify_keys(a["verts"], a["dtype"], a["V"], a["faces"], a["F"], a["cell"], _origin(a["origin"]), a["keys"], a["ws"],
                                      _ws_bytes(lib, a), None)


def _group(lib, **over):
    a = dict(skeys=PTR, order=PTR, V=V, scv=PTR, F=F, vclus=PTR, cstart=PTR, ccount=PTR, cbeg=PTR, cend=PTR, n=ctypes.c_long(-7), ws=PTR,
             ws_bytes=None)
    a.update(over)
    n = a["n"]
    return lib.dfh_mesh_simplify_group(a["skeys"], a["order"], a["V"], a["scv"], a["F"], a["vclus"], a["cstart"], a["ccount"], a["cbeg"], a["cend"],
                                       None if n is None else ctypes.byref(n), a["ws"], _ws_bytes(lib, a), None)


def _clusters(lib, **over):
    a = dict(verts=PTR, dtype=_lib.F64, V=V, faces=PTR, F=F, cell=1.0, origin=(0.0, 0.0, 0.0), mode=0, reg=1e-3, keys=PTR, order=PTR, corder=PTR,
             cbeg=PTR, cend=PTR, cstart=PTR, ccount=PTR, C=C, out=PTR, nfb=PTR, ws=PTR, ws_bytes=None)
    a.update(over)
    return lib.dfh_mesh_simplify_clusters(a["verts"], a["dtype"], a["V"], a["faces"], a["F"], a["cell"], _origin(a["origin"]), a["mode"], a["reg"],
                                          a["keys"], a["order"], a["corder"], a["cbeg"], a["cend"], a["cstart"], a["ccount"], a["C"], a["out"],
                                          a["nfb"], a["ws"], _ws_bytes(lib, a), None)


def _attr(lib, **over):
    a = dict(attr=PTR, dtype=_lib.F32, V=V, K=K, order=PTR, cstart=PTR, ccount=PTR, C=C, out=PTR)
    a.update(over)
    return lib.dfh_mesh_simplify_attr(a["attr"], a["dtype"], a["V"], a["K"], a["order"], a["cstart"], a["ccount"], a["C"], a["out"], None)


def _faces(lib, **over):
    a = dict(faces=PTR, V=V, F=F, vclus=PTR, C=C, drop=1, fout=PTR, fidx=PTR, cmap=PTR, kept=PTR, vmap=PTR, counts=(ctypes.c_long * 2)(-7, -7),
             ws=PTR, ws_bytes=None)
    a.update(over)
    return lib.dfh_mesh_simplify_faces(a["faces"], a["V"], a["F"], a["vclus"], a["C"], a["drop"], a["fout"], a["fidx"], a["cmap"], a["kept"],
                                       a["vmap"], a["counts"], a["ws"], _ws_bytes(lib, a), None)


SIZES = {
    "V negative": dict(V=-1),
    "V = 2^31": dict(V=1 << 31),
    "F negative": dict(F=-1),
    "F above (2^31 - 1) / 3": dict(F=((1 << 31) - 1) // 3 + 1),
}
WORKSPACE = {
    "null workspace": dict(ws=None),
    "misaligned workspace": dict(ws=PTR + 4),
    "workspace one byte short": dict(ws_bytes=-1),
    "workspace of nothing": dict(ws_bytes=0),
}
GRID = {
    "cell 0": dict(cell=0.0),
    "cell negative": dict(cell=-1.0),
    "cell NaN": dict(cell=NAN),
    "cell infinite": dict(cell=INF),
    "null origin": dict(origin=None),
    "origin NaN": dict(origin=(0.0, NAN, 0.0)),
    "origin infinite": dict(origin=(0.0, 0.0, -INF)),
    "unknown dtype": dict(dtype=2),
    "negative dtype": dict(dtype=-1),
}
CLUSTERS = {
    "C negative": dict(C=-1),
    "C above V": dict(C=V + 1),
}
KEYS_REFUSED = dict(SIZES, **WORKSPACE, **GRID, **{
    "null verts": dict(verts=None),
    "null faces": dict(faces=None),
    "null keys": dict(keys=None),
})
GROUP_REFUSED = dict(SIZES, **WORKSPACE, **{
    "null sorted_keys": dict(skeys=None),
    "null order": dict(order=None),
    "null sorted_corner_vert": dict(scv=None),
    "null vert_cluster": dict(vclus=None),
    "null cluster_start": dict(cstart=None),
    "null cluster_count": dict(ccount=None),
    "null corner_begin": dict(cbeg=None),
    "null corner_end": dict(cend=None),
    "null n_clusters": dict(n=None),
    "faces without vertices": dict(V=0),
})
CLUSTERS_REFUSED = dict(SIZES, **WORKSPACE, **GRID, **CLUSTERS, **{
    "unknown mode": dict(mode=2),
    "negative mode": dict(mode=-1),
    "reg negative": dict(reg=-1e-3),
    "reg NaN": dict(reg=NAN),
    "reg infinite": dict(reg=INF),
    "null verts": dict(verts=None),
    "null faces": dict(faces=None),
    "null keys": dict(keys=None),
    "null order": dict(order=None),
    "null corner_order": dict(corder=None),
    "null corner_begin": dict(cbeg=None),
    "null corner_end": dict(cend=None),
    "null cluster_start": dict(cstart=None),
    "null cluster_count": dict(ccount=None),
    "null verts_out": dict(out=None),
    "null n_fallback": dict(nfb=None),
})
ATTR_REFUSED = dict(CLUSTERS, **{
    "V negative": dict(V=-1),
    "V = 2^31": dict(V=1 << 31),
    "width negative": dict(K=-1),
    "width = 2^31": dict(K=1 << 31),
    "unknown dtype": dict(dtype=2),
    "negative dtype": dict(dtype=-1),
    "null attr": dict(attr=None),
    "null order": dict(order=None),
    "null cluster_start": dict(cstart=None),
    "null cluster_count": dict(ccount=None),
    "null out": dict(out=None),
})
FACES_REFUSED = dict(SIZES, **WORKSPACE, **CLUSTERS, **{
    "drop_unreferenced 2": dict(drop=2),
    "drop_unreferenced -1": dict(drop=-1),
    "null faces": dict(faces=None),
    "null vert_cluster": dict(vclus=None),
    "null faces_out": dict(fout=None),
    "null face_idx": dict(fidx=None),
    "null cluster_map": dict(cmap=None),
    "null kept_cluster_idx": dict(kept=None),
    "null vert_map": dict(vmap=None),
    "null counts_out": dict(counts=None),
    "faces without clusters": dict(C=0),
})


@pytest.mark.parametrize("what", sorted(KEYS_REFUSED))
@on_own_thread
def test_keys_refuses(lib, what):
    _refused(lib, _keys(lib, **KEYS_REFUSED[what]), "dfh_mesh_simplify_keys")


@pytest.mark.parametrize("what", sorted(GROUP_REFUSED))
@on_own_thread
def test_group_refuses(lib, what):
    n = ctypes.c_long(-7)
    over = dict(GROUP_REFUSED[what])
    over.setdefault("n", n)
    _refused(lib, _group(lib, **over), "dfh_mesh_simplify_group")
    assert n.value == -7                                    # nothing was written


@pytest.mark.parametrize("what", sorted(CLUSTERS_REFUSED))
@on_own_thread
def test_clusters_refuses(lib, what):
    _refused(lib, _clusters(lib, **CLUSTERS_REFUSED[what]), "dfh_mesh_simplify_clusters")


@pytest.mark.parametrize("what", sorted(ATTR_REFUSED))
@on_own_thread
def test_attr_refuses(lib, what):
    _refused(lib, _attr(lib, **ATTR_REFUSED[what]), "dfh_mesh_simplify_attr")


@pytest.mark.parametrize("what", sorted(FACES_REFUSED))
@on_own_thread
def test_faces_refuses(lib, what):
    counts = (ctypes.c_long * 2)(-7, -7)
    over = dict(FACES_REFUSED[what])
    over.setdefault("counts", counts)
    _refused(lib, _faces(lib, **over), "dfh_mesh_simplify_faces")
    assert list(counts) == [-7, -7]                          # nothing was written


@on_own_thread
def test_empty_meshes_are_valid_and_launch_nothing(lib):
    assert _keys(lib, V=0, F=0, verts=None, faces=None, keys=None, ws=None, ws_bytes=0) == OK
    n = ctypes.c_long(-7)
    assert _group(lib, V=0, F=0, skeys=None, order=None, scv=None, vclus=None, cstart=None, ccount=None, cbeg=None, cend=None, n=n, ws=None,
                  ws_bytes=0) == OK and n.value == 0
    assert _attr(lib, V=0, C=0, attr=None, order=None, cstart=None, ccount=None, out=None) == OK
    assert _attr(lib, K=0, attr=None, out=None) == OK
    counts = (ctypes.c_long * 2)(-7, -7)
    assert _faces(lib, V=0, F=0, C=0, faces=None, vclus=None, fout=None, fidx=None, cmap=None, kept=None, vmap=None, counts=counts, ws=None,
                  ws_bytes=0) == OK
    assert list(counts) == [0, 0]


def test_workspace_size(lib):
    size = lib.dfh_mesh_simplify_workspace_bytes
    assert size(-1, 0) == 0 and size(0, -1) == 0 and size(1 << 31, 0) == 0 and size(0, ((1 << 31) - 1) // 3 + 1) == 0
    assert size(0, 0) > 0 and size(0, 0) % 8 == 0
    assert size(1000, 2000) % 8 == 0 and size(1000, 2000) > size(1000, 1000) > size(10, 10)
    assert size(2000, 1000) > size(1000, 1000)
    last = 0
    for n in (0, 1, 7, 1023, 1024, 1025, 4096, 100_000):     # monotone in both counts
        assert size(n, n) > last and size(n + 1, n) >= size(n, n) and size(n, n + 1) >= size(n, n)
        last = size(n, n)
    assert size(800_000, 1_570_000) < 160 << 20             # the 512^3 scene mesh: 80 bytes a vertex of quadrics and the lists


PY_REFUSED = {
    "verts (V, 2)": (dict(cell=1.0), np.zeros((4, 2)), np.zeros((1, 3), dtype=np.int32)),
    "verts int": (dict(cell=1.0), np.zeros((4, 3), dtype=np.int64), np.zeros((1, 3), dtype=np.int32)),
    "faces (F, 4)": (dict(cell=1.0), np.zeros((4, 3)), np.zeros((1, 4), dtype=np.int32)),
    "faces float": (dict(cell=1.0), np.zeros((4, 3)), np.zeros((1, 3))),
    "cell 0": (dict(cell=0.0), np.zeros((4, 3)), np.zeros((1, 3), dtype=np.int32)),
    "cell NaN": (dict(cell=NAN), np.zeros((4, 3)), np.zeros((1, 3), dtype=np.int32)),
    "reg negative": (dict(cell=1.0, reg=-1.0), np.zeros((4, 3)), np.zeros((1, 3), dtype=np.int32)),
    "unknown mode": (dict(cell=1.0, mode="median"), np.zeros((4, 3)), np.zeros((1, 3), dtype=np.int32)),
    "integer attribute": (dict(cell=1.0), np.zeros((4, 3)), np.zeros((1, 3), dtype=np.int32), np.zeros(4, dtype=np.int32)),
    "short attribute": (dict(cell=1.0), np.zeros((4, 3)), np.zeros((1, 3), dtype=np.int32), np.zeros((3, 2))),
}


@pytest.mark.parametrize("what", sorted(PY_REFUSED))
def test_python_refuses_before_it_needs_a_gpu(lib, what):
    kw, *args = PY_REFUSED[what]
    with pytest.raises(ValueError):
        mesh.simplify(*args, **kw)


def test_the_new_entry_points_are_bound(lib):
    for name in NAMES:
        assert name in _lib._SIGNATURES and name in _lib.declared_symbols() and hasattr(lib, name)
    assert _lib.ABI_VERSION == 8 and lib.dfh_version() == 8
