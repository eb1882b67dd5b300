"""CPU: what the K1-K3 entry points that take a dfh_slab or a dfh_volume, and the point-query / residual / graph entry points of the
solve, do with arguments they cannot use.  Validation comes before any HIP call, so no GPU is needed: device pointers are dummy
non-null integers that nothing dereferences."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import pytest

from dynamicfusion_body_amd import _lib, build

OK, BADARG = 0, -1
PTR = 0x1000                                    # a "device pointer"
G = (4, 4, 4)
EYE8 = (ctypes.c_double * 8)(1.0)
OUT13 = (ctypes.c_size_t * 13)()

# name -> which bad slab
BAD_SLABS = {
    "res with a zero": ((4, 0, 4), (0, 4)),
    "x0 > x1": (G, (3, 2)),
    "x1 > res[0]": (G, (0, 5)),
    "65536 planes": ((70000, 4, 4), (0, 65536)),
}


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def _volume(slab, dtype=_lib.F32):
    return _lib.Volume(PTR, PTR, dtype, slab)


def _views(n=1):
    ptrs = (ctypes.c_void_p * 1)(PTR)
    eye = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    v = _lib.DepthViews(n, ptrs, _lib.F32, 8, 8, eye, eye, (ctypes.c_double * 12)(), 1.0, (ctypes.c_double * 3)(), 4)
    v.keep = ptrs
    return v


LIVE = _lib.Live(PTR, _lib.F32, _lib.iarr(G))
NODES = _lib.Nodes(PTR, PTR, PTR, 8, 4)
F12, F3 = (ctypes.c_float * 12)(), (ctypes.c_float * 3)()

# entry point -> call(lib, slab or None); the calls that take a dfh_volume come below
SLAB_CALLS = {
    "dfh_integrate_depth_path": lambda lib, s: lib.dfh_integrate_depth_path(_lib.F32, s, 8, 8, 1),
    "dfh_dqb_skip_layout": lambda lib, s: lib.dfh_dqb_skip_layout(s, _lib.iarr(G), 4, 8, OUT13),
    "dfh_dqb_build_candidates": lambda lib, s: lib.dfh_dqb_build_candidates(s, PTR, 8, 4, PTR, 1 << 20, None),
    "dfh_sample_knn_bricks": lambda lib, s: lib.dfh_sample_knn_bricks(PTR, 5, PTR, PTR, 8, 4, s, PTR, 1 << 20, PTR, PTR, None),
}
SIZE_QUERIES = {
    "dfh_integrate_workspace_bytes": lambda lib, s: lib.dfh_integrate_workspace_bytes(1, 8, 8, s),
    "dfh_dqb_workspace_bytes": lambda lib, s: lib.dfh_dqb_workspace_bytes(s),
    "dfh_dqb_workspace_bytes_cached": lambda lib, s: lib.dfh_dqb_workspace_bytes_cached(s, 4, 8, 2),
}
VOLUME_CALLS = {
    "dfh_integrate_depth": lambda lib, v: lib.dfh_integrate_depth(v, _views(), 0.1, 100.0, None, None, 0, None),
    "dfh_integrate_depth_ocl": lambda lib, v: lib.dfh_integrate_depth_ocl(v, PTR, 8, 8, F12, F3, 0.1, 100.0, None),
    "dfh_fuse_volume_rigid": lambda lib, v: lib.dfh_fuse_volume_rigid(v, LIVE, EYE8, 0.1, 100.0, None),
    "dfh_fuse_volume_dqb": lambda lib, v: lib.dfh_fuse_volume_dqb(v, LIVE, NODES, EYE8, 0.1, 100.0, PTR, 1 << 20, 1, None),
}


def on_own_thread(test):
    """dfh_last_error() is kept per thread: the refused calls are made on a thread of their own, so that the main thread's
    message stays what the tests that read it there expect."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        with ThreadPoolExecutor(1) as ex:
            return ex.submit(test, *args, **kwargs).result()
    return run


def _refused(lib, name, rc):
    assert rc == BADARG, (name, rc)
    assert name.encode() in lib.dfh_last_error(), (name, lib.dfh_last_error())


@pytest.mark.parametrize("name", sorted(SLAB_CALLS))
@on_own_thread
def test_slab_calls_refuse_bad_slabs(lib, name):
    _refused(lib, name, SLAB_CALLS[name](lib, None))
    for res, x_range in BAD_SLABS.values():
        _refused(lib, name, SLAB_CALLS[name](lib, _lib.slab(res, x_range)))
    assert SLAB_CALLS[name](lib, _lib.slab(G, (2, 2))) == OK


@pytest.mark.parametrize("name", sorted(SIZE_QUERIES))
@on_own_thread
def test_size_queries_give_zero(lib, name):
    assert SIZE_QUERIES[name](lib, None) == 0
    for res, x_range in BAD_SLABS.values():
        assert SIZE_QUERIES[name](lib, _lib.slab(res, x_range)) == 0, (name, res, x_range)
    assert SIZE_QUERIES[name](lib, _lib.slab(G, (2, 2))) == 0
    assert SIZE_QUERIES[name](lib, _lib.slab(G)) > 0


@pytest.mark.parametrize("name", sorted(VOLUME_CALLS))
@on_own_thread
def test_volume_calls_refuse_bad_volumes(lib, name):
    _refused(lib, name, VOLUME_CALLS[name](lib, None))
    for res, x_range in BAD_SLABS.values():
        _refused(lib, name, VOLUME_CALLS[name](lib, _volume(_lib.slab(res, x_range))))
    _refused(lib, name, VOLUME_CALLS[name](lib, _volume(_lib.slab(G), dtype=2)))
    assert VOLUME_CALLS[name](lib, _volume(_lib.slab(G, (2, 2)))) == OK


@on_own_thread
def test_integrate_depth_without_views(lib):
    """No views and no fresh value: nothing to do, on a full slab too (no launch); a fresh value on an empty slab likewise."""
    assert lib.dfh_integrate_depth(_volume(_lib.slab(G)), _views(0), 0.1, 100.0, None, None, 0, None) == OK
    assert lib.dfh_integrate_depth(_volume(_lib.slab(G, (2, 2))), _views(0), 0.1, 100.0, ctypes.c_double(0.1), None, 0, None) == OK
    _refused(lib, "dfh_integrate_depth", lib.dfh_integrate_depth(_volume(_lib.slab(G)), None, 0.1, 100.0, None, None, 0, None))
    _refused(lib, "dfh_integrate_depth", lib.dfh_integrate_depth(_volume(_lib.slab(G)), _views(17), 0.1, 100.0, None, None, 0, None))


# ---- the point-query, residual and graph entry points: sizes first, then "nothing to do", then pointers ----------------------
# call(lib, n, knn, m, ptr): n rows, m live vertices / cloud points / nodes, every pointer = ptr
POINT_CALLS = {
    "dfh_closest_correspondences": lambda lib, n, knn, m, p: lib.dfh_closest_correspondences(p, p, n, p, m, knn, 0.2, p, None, p, None),
    "dfh_nearest_points": lambda lib, n, knn, m, p: lib.dfh_nearest_points(p, n, p, m, p, None, None),
    "dfh_graph_unsupported": lambda lib, n, knn, m, p: lib.dfh_graph_unsupported(p, n, p, knn, p, p, m, p, None),
    "dfh_dq_blend_points": lambda lib, n, knn, m, p: lib.dfh_dq_blend_points(p, n, p, knn, p, p, p, m, p, None),
    "dfh_sample_knn": lambda lib, n, knn, m, p: lib.dfh_sample_knn(p, n, p, p, m, knn, p, p, None),
    "dfh_residual_data": lambda lib, n, knn, m, p: lib.dfh_residual_data(p, p, p, p, n, knn, p, p, p, m, EYE8 if p else None, p, None),
    "dfh_residual_reg": lambda lib, n, knn, m, p: lib.dfh_residual_reg(p, n, knn, p, p, p, 1.0, p, None),
    "dfh_warp_points": lambda lib, n, knn, m, p: lib.dfh_warp_points(p, p, p, n, knn, p, p, p, m, EYE8 if p else None, p, p, None),
    "dfh_permute_samples": lambda lib, n, knn, m, p: lib.dfh_permute_samples(p, n, knn, p, p, p, p, p, p, p, p, None),
}
NEEDS_M_GE_KNN = ("dfh_closest_correspondences", "dfh_sample_knn")          # knn neighbours out of m points
NEEDS_M_GE_1 = ("dfh_nearest_points", "dfh_graph_unsupported", "dfh_dq_blend_points", "dfh_residual_data")
NO_KNN = ("dfh_nearest_points",)


@pytest.mark.parametrize("name", sorted(POINT_CALLS))
@on_own_thread
def test_point_calls_refuse_bad_sizes_and_null_pointers(lib, name):
    call = POINT_CALLS[name]
    _refused(lib, name, call(lib, -1, 4, 8, PTR))                           # a negative count
    _refused(lib, name, call(lib, 5, 4, 8, None))                           # null pointers with a positive count
    if name not in NO_KNN:
        if name == "dfh_warp_points":                                       # (knn matters only with a neighbour table: it has one here)
            _refused(lib, name, call(lib, 5, 0, 8, PTR))
            _refused(lib, name, call(lib, 5, 9, 8, PTR))
        else:
            _refused(lib, name, call(lib, 0, 0, 8, PTR))                    # knn 0 and knn 9, refused even with nothing to do
            _refused(lib, name, call(lib, 0, 9, 16, PTR))
    if name in NEEDS_M_GE_KNN:
        _refused(lib, name, call(lib, 5, 4, 3, PTR))                        # n_live / n_nodes < knn
        _refused(lib, name, call(lib, 0, 4, 3, None))
        _refused(lib, name, call(lib, 5, 1, 0, PTR))
        _refused(lib, name, call(lib, 5, 4, -1, PTR))
    if name in NEEDS_M_GE_1:
        _refused(lib, name, call(lib, 5, 4, 0, PTR))                        # n_cloud = 0 / no nodes
        _refused(lib, name, call(lib, 0, 4, 0, None))
        _refused(lib, name, call(lib, 5, 4, -3, PTR))
    assert call(lib, 0, 4, 8, None) == OK                                   # a count of 0 with null pointers: nothing to do
    assert call(lib, 0, 8, 8, PTR) == OK and call(lib, 0, 1, 8, PTR) == OK  # (knn 8 and 1 are inside the range)


@on_own_thread
def test_warp_points_refuses_normals_out_without_normals(lib):
    _refused(lib, "dfh_warp_points", lib.dfh_warp_points(PTR, None, None, 5, 1, None, None, None, 0, EYE8, PTR, PTR, None))
    _refused(lib, "dfh_warp_points", lib.dfh_warp_points(PTR, PTR, PTR, 5, 4, PTR, PTR, PTR, 0, EYE8, PTR, PTR, None))      # a table, no nodes
    _refused(lib, "dfh_warp_points", lib.dfh_warp_points(PTR, PTR, PTR, 5, 4, None, PTR, PTR, 8, EYE8, PTR, PTR, None))
    _refused(lib, "dfh_warp_points", lib.dfh_warp_points(PTR, PTR, None, 5, 4, None, None, None, 0, None, PTR, PTR, None))  # no lw_dq


@pytest.mark.parametrize("name", ["dfh_gn_pack_upper", "dfh_gn_unpack_upper"])
@on_own_thread
def test_pack_upper_refuses_bad_arguments(lib, name):
    fn = getattr(lib, name)
    _refused(lib, name, fn(None, None, None, None, 0, 0, 0, None, None))     # (these two always launch: no "nothing to do" form)
    for i in range(4):
        ptrs = [PTR] * 4
        ptrs[i] = None
        _refused(lib, name, fn(*ptrs, 4, 2, 3, PTR, None))
    _refused(lib, name, fn(PTR, PTR, PTR, PTR, 4, 2, 3, None, None))
    for counts in ((-1, 2, 3), (4, -1, 3), (4, 2, -1)):
        _refused(lib, name, fn(PTR, PTR, PTR, PTR, *counts, PTR, None))


# ---- the block-Jacobi PCG: sizes, pointers and the workspace are checked before anything is launched or written -----------------
def _pcg_buffers(n=4, iters=3):
    """Host arrays standing in for the device buffers (a refused call dereferences none): a 4-row diagonal system, x_out,
    node_dq and a workspace of exactly the size the library asks for, each filled with a pattern."""
    ws_bytes = 8 * (36 * n + 30 * n + 3 * (iters + 2) + 2 * (iters + 1) * ((n + 3) // 4) + 72 * n)
    b = {
        "row_ptr": (ctypes.c_int * (n + 1))(*range(n + 1)),
        "col": (ctypes.c_int * n)(*range(n)),
        "vals": (ctypes.c_double * (36 * n))(*([2.5] * (36 * n))),
        "rhs": (ctypes.c_double * (6 * n))(*([1.5] * (6 * n))),
        "x": (ctypes.c_double * (6 * n))(*([-7.25] * (6 * n))),
        "ws": (ctypes.c_ubyte * ws_bytes)(*([0xA5] * ws_bytes)),
        "dq": (ctypes.c_double * (8 * n))(*([0.125] * (8 * n))),
    }
    return b, ws_bytes


def _pcg_call(lib, update, b, n, iters, ws_bytes, null=None):
    p = {k: (None if k == null else ctypes.addressof(v)) for k, v in b.items()}
    args = (p["row_ptr"], p["col"], p["vals"], p["rhs"], n, iters, 1e-3, 1e-2, p["x"], p["ws"], ws_bytes)
    if update:
        return lib.dfh_pcg_solve_update(*args, p["dq"], 1.0, None)
    return lib.dfh_pcg_solve(*args, None)


@pytest.mark.parametrize("update", [False, True])
@on_own_thread
def test_pcg_solve_refuses_bad_arguments_and_writes_nothing(lib, update):
    n, iters = 4, 3
    b, ws_bytes = _pcg_buffers(n, iters)
    assert lib.dfh_pcg_workspace_bytes(n, iters) == ws_bytes
    before = {k: bytes(v) for k, v in b.items()}
    name = "dfh_pcg_solve"                                                  # (dfh_pcg_solve_update reports under both names)

    def refused(rc, what=name):
        _refused(lib, what, rc)
        assert {k: bytes(v) for k, v in b.items()} == before                # nothing was written, the matrix's damping included

    refused(_pcg_call(lib, update, b, 0, iters, ws_bytes))                  # no rows
    refused(_pcg_call(lib, update, b, -3, iters, ws_bytes))
    refused(_pcg_call(lib, update, b, n, 0, ws_bytes))                      # no iterations
    refused(_pcg_call(lib, update, b, n, -1, ws_bytes))
    for null in ("row_ptr", "col", "vals", "rhs", "x", "ws"):
        refused(_pcg_call(lib, update, b, n, iters, ws_bytes, null=null))
    if update:
        refused(_pcg_call(lib, update, b, n, iters, ws_bytes, null="dq"), "dfh_pcg_solve_update")
    refused(_pcg_call(lib, update, b, n, iters, ws_bytes - 1))              # a workspace one byte short
    refused(_pcg_call(lib, update, b, n, iters + 1, ws_bytes))              # ... or sized for fewer iterations
    refused(_pcg_call(lib, update, b, n, iters, 0))


@on_own_thread
def test_pcg_queries_refuse_bad_sizes(lib):
    _refused(lib, "dfh_pcg_path", lib.dfh_pcg_path(0))
    _refused(lib, "dfh_pcg_path", lib.dfh_pcg_path(-5))
    assert lib.dfh_pcg_workspace_bytes(0, 10) == 0 and lib.dfh_pcg_workspace_bytes(-1, 10) == 0 and lib.dfh_pcg_workspace_bytes(4, -1) == 0
    _refused(lib, "dfh_pcg_set_mode", lib.dfh_pcg_set_mode(1))
    _refused(lib, "dfh_pcg_set_mode", lib.dfh_pcg_set_mode(3))
