"""CPU: the numpy restatement of dfh_nearest_descriptors against scipy's KD-tree, the entry point's argument checks (they come
before any HIP call: device pointers are dummy non-null integers that nothing dereferences), the nd_path option, and the shape
checks of the Python layers."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import descriptors_np as DN
from dynamicfusion_body_amd import Fusion, _lib, build, graph, solve

OK, BADARG = 0, -1
PTR = 0x1000                                    # a "device pointer" (16-byte aligned)
NAME = b"dfh_nearest_descriptors"


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


@pytest.mark.parametrize("dim,nq,nb,seed", [(1, 40, 50, 0), (3, 64, 257, 1), (16, 100, 300, 2), (64, 33, 129, 3)])
def test_restatement_agrees_with_ckdtree(dim, nq, nb, seed):
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    b = rng.standard_normal((nb, dim)).astype(np.float32)
    idx, d2 = DN.nearest_descriptors(q, b)
    dist, ref = cKDTree(b.astype(np.float64)).query(q.astype(np.float64))
    full = DN.d2_matrix(q, b)
    assert (np.sort(full, axis=1)[:, 1] > np.sort(full, axis=1)[:, 0]).all()         # tie-free, so the tree's rule does not matter
    assert np.array_equal(idx, ref.astype(np.int32))
    np.testing.assert_allclose(np.sqrt(d2), dist, rtol=1e-14, atol=0)


def test_restatement_ties_and_bad_values():
    b = np.array([[1, 0], [0, 1], [1, 0], [np.nan, 0], [np.inf, 0]], dtype=np.float32)
    q = np.array([[0, 0], [1, 0], [np.nan, 1], [-np.inf, 0]], dtype=np.float32)
    idx, d2 = DN.nearest_descriptors(q, b)
    assert idx.tolist() == [0, 0, -1, -1]
    assert d2.tolist() == [1.0, 0.0, np.inf, np.inf]
    idx, d2 = DN.nearest_descriptors(q[:2], b[3:])
    assert idx.tolist() == [-1, -1] and np.isposinf(d2).all()


def _call(lib, query=PTR, nq=10, base=PTR, nb=20, dim=16, idx=PTR, d2=PTR, stats=PTR, ws=PTR, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return lib.dfh_nearest_descriptors(query, nq, base, nb, dim, idx, d2, stats, ws, ws_bytes, None)


BAD = {
    "dim 0": dict(dim=0),
    "dim 65": dict(dim=65),
    "dim < 0": dict(dim=-3),
    "n_base 0": dict(nb=0),
    "n_base < 0": dict(nb=-1),
    "n_base 2^31": dict(nb=2 ** 31),
    "n_query < 0": dict(nq=-1),
    "n_query 2^31": dict(nq=2 ** 31),
    "null query": dict(query=None),
    "null base": dict(base=None),
    "null idx_out": dict(idx=None),
    "dim 0 with n_query 0": dict(dim=0, nq=0),
    "n_base 0 with n_query 0": dict(nb=0, nq=0),
}
BAD_FAST = {                                    # the fast path's workspace (the exact kernel has none)
    "null workspace": dict(ws=None),
    "misaligned workspace": dict(ws=PTR + 4),
    "workspace one byte short": "short",
    "workspace of 0 bytes": dict(ws_bytes=0),
}


@pytest.mark.parametrize("path", [None, 1, 2])
@pytest.mark.parametrize("what", sorted(BAD))
@on_own_thread
def test_bad_arguments_are_refused_before_any_launch(lib, what, path):
    _lib.set_option("nd_path", path)
    rc = _call(lib, **BAD[what])
    assert rc == BADARG, (what, rc)
    assert NAME in lib.dfh_last_error(), (what, lib.dfh_last_error())


@pytest.mark.parametrize("what", sorted(BAD_FAST))
@on_own_thread
def test_fast_path_refuses_a_bad_workspace(lib, what):
    _lib.set_option("nd_path", 2)
    kw = BAD_FAST[what]
    if kw == "short":
        kw = dict(ws_bytes=lib.dfh_nearest_descriptors_workspace_bytes(10, 20, 16) - 1)
    rc = _call(lib, **kw)
    assert rc == BADARG, (what, rc)
    assert NAME in lib.dfh_last_error() and b"workspace" in lib.dfh_last_error()


@on_own_thread
def test_size_queries(lib):
    f = lib.dfh_nearest_descriptors_workspace_bytes
    assert f(0, 20, 16) == 0 and f(10, 0, 16) == 0 and f(10, 20, 0) == 0 and f(10, 20, 65) == 0 and f(-1, 20, 16) == 0
    assert f(10, 20, 16) > 0 and f(10, 20, 16) % 16 == 0
    sizes = [f(n, 1000, 16) for n in (1, 127, 128, 129, 10 ** 4, 10 ** 6)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert f(1000, 1000, 16) <= f(1000, 1000, 17) <= f(1000, 1000, 64)
    for bad in ((10, 20, 0), (10, 20, 65), (10, 0, 16), (-1, 20, 16), (10, -1, 16)):
        rc = lib.dfh_nearest_descriptors_path(*bad)
        assert rc == BADARG and b"dfh_nearest_descriptors_path" in lib.dfh_last_error(), bad
    tile = (ctypes.c_int * 4)()
    assert lib.dfh_nearest_descriptors_tile(tile) == OK and all(t > 0 for t in tile)
    assert lib.dfh_nearest_descriptors_tile(None) == BADARG


@on_own_thread
def test_no_queries_is_ok_without_a_launch(lib):
    for path in (None, 1, 2):
        _lib.set_option("nd_path", path)
        assert _call(lib, nq=0, query=None, idx=None, d2=None, stats=None, ws=None, ws_bytes=0) == OK
        assert _call(lib, nq=0) == OK


@on_own_thread
def test_nd_path_option_round_trips(lib):
    assert _lib.get_option("nd_path") == -1
    for v in (1, 2):
        _lib.set_option("nd_path", v)
        assert _lib.get_option("nd_path") == v
        assert lib.dfh_nearest_descriptors_path(10, 20, 16) == v
        assert lib.dfh_nearest_descriptors_path(10 ** 6, 10 ** 6, 16) == v
    _lib.set_option("nd_path", 3)                                           # not a path: the call refuses, the query falls back
    assert _call(lib) == BADARG and b"nd_path" in lib.dfh_last_error()
    _lib.set_option("nd_path", None)
    assert _lib.get_option("nd_path") == -1
    assert lib.dfh_nearest_descriptors_path(10, 20, 16) in (1, 2)


def test_python_wrapper_refuses_before_the_device():
    f32 = np.zeros((4, 16), dtype=np.float32)
    with pytest.raises(ValueError, match="width"):
        solve.nearest_descriptors(f32, np.zeros((5, 15), dtype=np.float32))
    with pytest.raises(ValueError, match="channels"):
        solve.nearest_descriptors(np.zeros((4, 65), dtype=np.float32), np.zeros((5, 65), dtype=np.float32))
    with pytest.raises(ValueError, match="no base"):
        solve.nearest_descriptors(f32, np.zeros((0, 16), dtype=np.float32))
    with pytest.raises(ValueError, match=r"\(n, D\)"):
        solve.nearest_descriptors(np.zeros(16, dtype=np.float32), f32)
    with pytest.raises(ValueError, match="float32-exact"):
        solve.nearest_descriptors(np.full((4, 16), 0.1), f32)              # 0.1 is not a float32
    with pytest.raises(ValueError, match="float32 or float64"):
        solve.nearest_descriptors(np.zeros((4, 16), dtype=np.int32), f32)


def _fusion_with_mesh(n=6):
    fu = Fusion(np.zeros((4, 4, 4)), 1.0, knn=4, write_warpfield=False)
    fu._vertices = np.arange(3 * n, dtype=np.float64).reshape(n, 3)
    fu._normals = np.tile([0.0, 0.0, 1.0], (n, 1))
    fu._neighbor_look_up = np.zeros((n, 4), dtype=np.int64)
    fu._nodes = [(i, fu._vertices[i], graph.NEW_NODE_DQ, 2.0) for i in range(4)]
    return fu


def test_setup_correspondences_refuses_mismatched_descriptors_before_the_device():
    fu = _fusion_with_mesh(6)
    live = np.zeros((9, 3))
    vol = np.zeros((4, 4, 4))
    ok_s, ok_l = np.zeros((6, 16), dtype=np.float32), np.zeros((9, 16), dtype=np.float32)
    cases = {
        "s_feats rows": (np.zeros((5, 16), dtype=np.float32), ok_l),
        "l_feats rows": (ok_s, np.zeros((8, 16), dtype=np.float32)),
        "widths": (ok_s, np.zeros((9, 15), dtype=np.float32)),
        "too wide": (np.zeros((6, 65), dtype=np.float32), np.zeros((9, 65), dtype=np.float32)),
        "not 2-D": (np.zeros(6, dtype=np.float32), ok_l),
    }
    for what, pair in cases.items():
        with pytest.raises(ValueError):
            fu.setupCorrespondences(vol, method='cnn', descriptors=pair, live_vertices=live)
        assert len(fu._vertices) == 6 and len(fu._correspondences) == 0, what
    with pytest.raises(ValueError, match="pair"):
        fu.setupCorrespondences(vol, method='cnn', descriptors=(ok_s,), live_vertices=live)
    assert Fusion.descriptor_fn is None
