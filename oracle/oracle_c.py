"""ctypes loader of oracle/liboracle_c.so (the C restatement of A1, A3 and A4) -- TEST INFRASTRUCTURE ONLY."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "liboracle_c.so")
_lib = None


def build(force=False):
    src = os.path.join(HERE, "oracle_c.c")
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(src):
        subprocess.run(["make", "-C", HERE, "-B", "liboracle_c.so"], check=True, capture_output=True)
    return LIB


def load():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        _lib.oracle_c_fuse_depths.restype = ctypes.c_long
        _lib.oracle_c_threads.restype = ctypes.c_int
        for name in ("oracle_c_update_tsdf_rigid", "oracle_c_update_tsdf_rigid_list", "oracle_c_update_tsdf_dqb",
                     "oracle_c_update_tsdf_dqb_list"):
            getattr(_lib, name).restype = ctypes.c_long
    return _lib


def threads():
    return int(load().oracle_c_threads())


def fuse_depths(dm, lw, K, Kinv, tsdf, tsdf_w, tdist, tsdf_res=None, scale=1.0, center=np.zeros(3), wmax=100.0,
                x_range=None, n_threads=0):
    """Same contract as oracle_np.fuse_depths (in place on float64 C-contiguous volumes)."""
    lib = load()
    assert tsdf.dtype == np.float64 and tsdf_w.dtype == np.float64 and tsdf.flags.c_contiguous and tsdf_w.flags.c_contiguous
    dm = np.ascontiguousarray(dm)
    if dm.dtype not in (np.float32, np.float64):
        dm = dm.astype(np.float64)
    X, Y, Z = tsdf.shape
    a, b = (0, X) if x_range is None else x_range
    dp = lambda arr: np.ascontiguousarray(np.asarray(arr, dtype=np.float64)).ctypes.data_as(ctypes.c_void_p)
    Kc, Kic, lwc, cc = (np.ascontiguousarray(np.asarray(v, dtype=np.float64)) for v in (K, Kinv, lw, center))
    n = lib.oracle_c_fuse_depths(tsdf.ctypes.data_as(ctypes.c_void_p), tsdf_w.ctypes.data_as(ctypes.c_void_p),
                                 ctypes.c_int(X), ctypes.c_int(Y), ctypes.c_int(Z),
                                 ctypes.c_int(X if tsdf_res is None else int(tsdf_res)), ctypes.c_int(a), ctypes.c_int(b),
                                 dm.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(1 if dm.dtype == np.float32 else 0),
                                 ctypes.c_int(dm.shape[0]), ctypes.c_int(dm.shape[1]),
                                 Kc.ctypes.data_as(ctypes.c_void_p), Kic.ctypes.data_as(ctypes.c_void_p),
                                 lwc.ctypes.data_as(ctypes.c_void_p), ctypes.c_double(scale),
                                 cc.ctypes.data_as(ctypes.c_void_p), ctypes.c_double(tdist), ctypes.c_double(wmax),
                                 ctypes.c_int(n_threads))
    return int(n)


# ------------------------------------------------------------------------------------------------ A3 / A4: TSDF -> TSDF fusion
def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _f64(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if shape is not None and a.shape != shape:
        raise ValueError("array of shape %s, expected %s" % (a.shape, shape))
    return a


def _live(curr_tsdf):
    """The live volume as the C side reads it: float32 or float64 in place (no copy when already C-contiguous)."""
    live = np.asarray(curr_tsdf)
    if live.ndim != 3:
        raise ValueError("live TSDF must be 3-D")
    if live.dtype not in (np.float32, np.float64):
        live = live.astype(np.float64)
    live = np.ascontiguousarray(live)
    return live, ctypes.c_int(1 if live.dtype == np.float32 else 0), (ctypes.c_int * 3)(*live.shape)


def _nodes(node_pos, node_dq, node_w, knn):
    P = _f64(node_pos).reshape(-1, 3)
    N = P.shape[0]
    Q, Wn = _f64(node_dq, (N, 8)), _f64(node_w, (N,))
    if not (1 <= int(knn) <= 8 and N >= int(knn)):
        raise ValueError("knn must be in [1, 8] and at most the number of nodes")
    return P, Q, Wn, N


def _volume_args(tsdf, tsdf_w, x_range, x_base):
    if not (tsdf.dtype == np.float64 and tsdf_w.dtype == np.float64 and tsdf.flags.c_contiguous and tsdf_w.flags.c_contiguous
            and tsdf.ndim == 3 and tsdf.shape == tsdf_w.shape):
        raise ValueError("tsdf / tsdf_w must be C-contiguous float64 volumes of one shape")
    nx, Y, Z = tsdf.shape
    a, b = (x_base, x_base + nx) if x_range is None else x_range
    if not (x_base <= a <= b <= x_base + nx):
        raise ValueError("x_range %s outside the planes [%d, %d) the volumes hold" % ((a, b), x_base, x_base + nx))
    return nx, Y, Z, a, b


def _list_args(idx, res, T_in, W_in):
    idx = np.ascontiguousarray(np.asarray(idx, dtype=np.int64).reshape(-1))
    n = idx.size
    T_in, W_in = _f64(T_in).reshape(-1), _f64(W_in).reshape(-1)
    if T_in.size != n or W_in.size != n:
        raise ValueError("T_in / W_in must hold one value per listed voxel")
    if n and (idx.min() < 0 or idx.max() >= int(np.prod(res))):
        raise ValueError("voxel index outside the grid")
    out = (np.empty(n), np.empty(n), np.empty(n, dtype=np.uint8))
    return idx, n, T_in, W_in, out


def update_tsdf_rigid(tsdf, tsdf_w, curr_tsdf, lw_dq, tdist, wmax=100.0, x_range=None, x_base=0, return_mask=False, n_threads=0):
    """Same contract as oracle_np.update_tsdf_rigid, in place on float64 C-contiguous volumes.  The volumes hold planes
    [x_base, x_base + tsdf.shape[0]) of the canonical grid (default: all of it); planes x_range (global indices) are swept.
    curr_tsdf: float32 or float64, any extent, read in place.  Returns the number of updated voxels (and the update mask)."""
    lib = load()
    nx, Y, Z, a, b = _volume_args(tsdf, tsdf_w, x_range, x_base)
    live, l32, lres = _live(curr_tsdf)
    mask = np.zeros(tsdf.shape, dtype=np.uint8) if return_mask else None
    n = lib.oracle_c_update_tsdf_rigid(_ptr(tsdf), _ptr(tsdf_w), _ptr(mask) if return_mask else None, ctypes.c_int(x_base),
                                       ctypes.c_int(nx), ctypes.c_int(Y), ctypes.c_int(Z), ctypes.c_int(a), ctypes.c_int(b), _ptr(live),
                                       l32, lres, _ptr(_f64(lw_dq, (8,))), ctypes.c_double(tdist), ctypes.c_double(wmax),
                                       ctypes.c_int(n_threads))
    return (int(n), mask.view(bool)) if return_mask else int(n)


def update_tsdf_rigid_at(idx, res, T_in, W_in, curr_tsdf, lw_dq, tdist, wmax=100.0, n_threads=0):
    """update_tsdf_rigid on the listed voxels only: idx = flat indices (x * Y + y) * Z + z of the `res` grid, T_in / W_in their
    values before the call.  Returns (T_out, W_out, mask) per listed voxel; exactly what the whole-volume form gives there."""
    lib = load()
    idx, n, T_in, W_in, (To, Wo, m) = _list_args(idx, res, T_in, W_in)
    live, l32, lres = _live(curr_tsdf)
    rc = lib.oracle_c_update_tsdf_rigid_list(_ptr(idx), ctypes.c_long(n), (ctypes.c_int * 3)(*res), _ptr(T_in), _ptr(W_in), _ptr(To),
                                             _ptr(Wo), _ptr(m), _ptr(live), l32, lres, _ptr(_f64(lw_dq, (8,))), ctypes.c_double(tdist),
                                             ctypes.c_double(wmax), ctypes.c_int(n_threads))
    assert rc >= 0
    return To, Wo, m.view(bool)


def update_tsdf_dqb(tsdf, tsdf_w, curr_tsdf, node_pos, node_dq, node_w, knn, lw_dq, tdist, wmax=100.0, x_range=None, x_base=0,
                    return_mask=False, n_threads=0):
    """Same contract as oracle_np.update_tsdf_dqb (and the volume / live arguments of update_tsdf_rigid above)."""
    lib = load()
    nx, Y, Z, a, b = _volume_args(tsdf, tsdf_w, x_range, x_base)
    live, l32, lres = _live(curr_tsdf)
    P, Q, Wn, N = _nodes(node_pos, node_dq, node_w, knn)
    mask = np.zeros(tsdf.shape, dtype=np.uint8) if return_mask else None
    n = lib.oracle_c_update_tsdf_dqb(_ptr(tsdf), _ptr(tsdf_w), _ptr(mask) if return_mask else None, ctypes.c_int(x_base),
                                     ctypes.c_int(nx), ctypes.c_int(Y), ctypes.c_int(Z), ctypes.c_int(a), ctypes.c_int(b), _ptr(live),
                                     l32, lres, _ptr(P), _ptr(Q), _ptr(Wn), ctypes.c_int(N), ctypes.c_int(int(knn)),
                                     _ptr(_f64(lw_dq, (8,))), ctypes.c_double(tdist), ctypes.c_double(wmax), ctypes.c_int(n_threads))
    assert n >= 0
    return (int(n), mask.view(bool)) if return_mask else int(n)


def update_tsdf_dqb_at(idx, res, T_in, W_in, curr_tsdf, node_pos, node_dq, node_w, knn, lw_dq, tdist, wmax=100.0, n_threads=0):
    """update_tsdf_dqb on the listed voxels only (see update_tsdf_rigid_at)."""
    lib = load()
    idx, n, T_in, W_in, (To, Wo, m) = _list_args(idx, res, T_in, W_in)
    live, l32, lres = _live(curr_tsdf)
    P, Q, Wn, N = _nodes(node_pos, node_dq, node_w, knn)
    rc = lib.oracle_c_update_tsdf_dqb_list(_ptr(idx), ctypes.c_long(n), (ctypes.c_int * 3)(*res), _ptr(T_in), _ptr(W_in), _ptr(To),
                                           _ptr(Wo), _ptr(m), _ptr(live), l32, lres, _ptr(P), _ptr(Q), _ptr(Wn), ctypes.c_int(N),
                                           ctypes.c_int(int(knn)), _ptr(_f64(lw_dq, (8,))), ctypes.c_double(tdist), ctypes.c_double(wmax),
                                           ctypes.c_int(n_threads))
    assert rc >= 0
    return To, Wo, m.view(bool)
