"""numpy restatement of the visible-surface samples of csrc/dfh_render.hip (semantics: include/dfusion_hip.h,
dfh_render_samples_*), on top of the rasterizer's restatement (tests/render_np.py: project, setup, bary).

The lattice pixels (every `stride`-th pixel of every `stride`-th row, view-major, then y, then x) that the face map of
render_np.render covers yield one sample each.  The weights are evaluated for all pixels of one (view, face) pair at once:
numpy's element-wise fp64 `+ * / sqrt` round like the kernel's scalar ones (no fused multiply-add), and every expression is
written in the kernel's operation order, so positions, normals and pixel indices agree bit for bit.
"""
import numpy as np

import render_np as RN


def subsample_index(total, capacity):
    """Indices of the samples the capacity rule keeps, in slot order: sample i is kept iff it is the first with slot
    floor(i * capacity / total), i.e. i = ceil(slot * total / capacity) (the index formula of extract_surface_samples_torch)."""
    total, capacity = int(total), int(capacity)
    if capacity >= total:
        return np.arange(total, dtype=np.int64)
    if capacity == 0:
        return np.zeros(0, dtype=np.int64)
    return (np.arange(capacity, dtype=np.int64) * total + capacity - 1) // capacity


def weights(u, v, z, A, xs, ys):
    """b0, b1, b2 of the header at pixel centres (xs, ys) of one projected triangle."""
    _, l0, l1, l2 = RN.bary(u, v, A, xs, ys)
    a0, a1, a2 = l0 / z[0], l1 / z[1], l2 / z[2]
    s = (a0 + a1) + a2
    return a0 / s, a1 / s, a2 / s


def render_samples(verts, faces, canon_pos, canon_nrm, K, lws, H, W, scale=1.0, center=0.0, half=0.0, znear=1e-3, stride=1,
                   max_samples=None, face_map=None):
    """Same call shape and results as mesh.render_samples, as numpy arrays: (pos (S,3) f64, nrm (S,3) f64 or None,
    pixel (S,) int64).  face_map: the (V,H,W) face map of render_np.render for these arguments, if the caller has it already
    (the map does not depend on the stride)."""
    verts = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    canon_pos = np.asarray(canon_pos, dtype=np.float64)
    canon_nrm = None if canon_nrm is None else np.asarray(canon_nrm, dtype=np.float64)
    lws = np.asarray(lws, dtype=np.float64)
    if lws.ndim == 2:
        lws = lws[None]
    nv = len(lws)
    if face_map is None:
        face_map = RN.render(verts, faces, None, K, lws, H, W, scale=scale, center=center, half=half, znear=znear)[2]
    lattice = np.zeros((nv, H, W), dtype=bool)
    lattice[:, ::stride, ::stride] = True
    vi, ys, xs = np.nonzero(lattice & (face_map >= 0))                # C order: view-major, then y, then x
    fs = face_map[vi, ys, xs].astype(np.int64)
    n = len(vi)
    pos = np.zeros((n, 3))
    m = np.zeros((n, 3))
    with np.errstate(all="ignore"):
        for view in range(nv):
            U, Vv, Z = RN.project(verts, K, lws[view], scale, center, half)
            in_view = vi == view
            for f in np.unique(fs[in_view]):
                sel = np.nonzero(in_view & (fs == f))[0]
                idx = faces[f]
                u, v, z = U[idx], Vv[idx], Z[idx]
                A = RN.setup(u, v, z, H, W, znear)[0]
                b0, b1, b2 = weights(u, v, z, A, xs[sel].astype(np.float64), ys[sel].astype(np.float64))
                for c in range(3):
                    pos[sel, c] = (b0 * canon_pos[idx[0], c] + b1 * canon_pos[idx[1], c]) + b2 * canon_pos[idx[2], c]
                    if canon_nrm is not None:
                        m[sel, c] = (b0 * canon_nrm[idx[0], c] + b1 * canon_nrm[idx[1], c]) + b2 * canon_nrm[idx[2], c]
        nrm = None
        if canon_nrm is not None:
            ln = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
            ok = (ln > 0) & np.isfinite(ln)
            nrm = np.where(ok[:, None], m / np.where(ok, ln, 1.0)[:, None], 0.0)
    pixel = (vi.astype(np.int64) * H + ys) * W + xs
    if max_samples is not None and int(max_samples) < n:
        keep = subsample_index(n, max_samples)
        pos, pixel = pos[keep], pixel[keep]
        nrm = None if nrm is None else nrm[keep]
    return pos, nrm, pixel
