"""numpy restatement of dfh_nearest_descriptors' definition (include/dfusion_hip.h, K14), and of the float32 score the fast
path filters with.  Accumulating (A[:, None, c] - B[None, :, c])**2 over c in order gives the sequential fp64 sum's bits:
numpy rounds every element-wise operation once and never contracts."""
import numpy as np


def d2_matrix(query, base):
    """(n_query, n_base) fp64: (((t_0*t_0) + t_1*t_1) + ...) with t_c = (double)query[q][c] - (double)base[l][c]."""
    A = np.asarray(query, dtype=np.float32).astype(np.float64)
    B = np.asarray(base, dtype=np.float32).astype(np.float64)
    assert A.ndim == 2 and B.ndim == 2 and A.shape[1] == B.shape[1]
    with np.errstate(all="ignore"):
        t = A[:, None, 0] - B[None, :, 0]
        d2 = t * t
        for c in range(1, A.shape[1]):
            t = A[:, None, c] - B[None, :, c]
            d2 = d2 + t * t
    return d2


def nearest_descriptors(query, base, block=2048):
    """(idx int32, d2 fp64): the counting (finite) pair with the smallest d2, lowest index on ties; -1 / +inf without one."""
    query = np.asarray(query, dtype=np.float32)
    idx = np.empty(len(query), dtype=np.int32)
    best = np.empty(len(query), dtype=np.float64)
    for q0 in range(0, len(query), block):
        d2 = d2_matrix(query[q0:q0 + block], base)
        d2 = np.where(np.isfinite(d2), d2, np.inf)
        arg = np.argmin(d2, axis=1)                      # (the first of equal minima: the lowest index)
        val = d2[np.arange(len(arg)), arg]
        idx[q0:q0 + block] = np.where(np.isfinite(val), arg, -1)
        best[q0:q0 + block] = val
    return idx, best


def f32_scores(query, base):
    """(n_query, n_base) float32: |b|^2 - 2 a.b as a k-ordered float32 chain -- products rounded, then added (the device fuses
    each product into its addition; this restatement is for counting distinct scores, not for bits)."""
    A = np.asarray(query, dtype=np.float32)
    B = np.asarray(base, dtype=np.float32)
    nb = (B.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    acc = np.zeros((len(A), len(B)), dtype=np.float32)
    for c in range(A.shape[1]):
        acc = acc + (np.float32(-2.0) * A[:, None, c]) * B[None, :, c]
    return acc + nb[None, :]
