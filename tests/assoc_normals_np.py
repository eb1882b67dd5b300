"""numpy restatement of the normal-compatibility gate of the depth data term (include/dfusion_hip.h: dfh_gn_normal_gate), the
oracle of tests/test_assoc_normals_cpu.py and tests/test_gpu_assoc_normals.py.

Built on oracle.gn_np.associate_depth (a view's correspondence) and oracle.oracle_np.warp(..., normal=...) (the sample's warped
normal n', as the data row warps it), with the comparison order of gn_np.associate_depth_views: the gate sits beside the distance
gate, in front of "smallest |c - x'|^2 wins, ties to the lower view"."""
import numpy as np

from oracle import gn_np
from oracle import oracle_np as O

EDGE = 1e-9          # relative margin inside which a gate decision may legitimately differ between two roundings


def warped(pos, nrm, dqs, nbr, node_pos, node_w, lw):
    """(x', n') of every sample: Fusion.warp with the sample's k node DQs, then the global lw."""
    return O.warp(pos, dqs[nbr], node_pos[nbr], node_w[nbr], normal=nrm, m_lw=lw)


def gate_terms(points_idx, normals_w, K, lw_cam, nmap, scale, center, half):
    """d, mm, ll of every sample against ONE view (steps 2 of the header's statement) and whether the sample projects inside the
    image at all (outside: the three are zero).  nmap: (H, W, 3) float32."""
    P = np.asarray(points_idx, dtype=np.float64)
    N = np.asarray(normals_w, dtype=np.float64)
    H, W = nmap.shape[:2]
    R, t = lw_cam[:, :3], lw_cam[:, 3]
    cam = (scale * (P - half) + center) @ R.T + t                   # (gn_np.associate_depth's projection, to the same pixel)
    u, v, ok = O.project_to_pixel(K, cam)
    vis = ok & (u >= 0) & (u < W - 1) & (v >= 0) & (v < H - 1)
    ui = np.where(vis, np.rint(u), 0).astype(np.int64)
    vi = np.where(vis, np.rint(v), 0).astype(np.int64)
    with np.errstate(all="ignore"):
        l = np.where(vis[:, None], nmap[vi, ui].astype(np.float64), 0.0)
        m = [(R[i, 0] * N[:, 0] + R[i, 1] * N[:, 1]) + R[i, 2] * N[:, 2] for i in range(3)]
        sgn = 1.0 if scale > 0 else -1.0
        d = sgn * ((m[0] * l[:, 0] + m[1] * l[:, 1]) + m[2] * l[:, 2])
        mm = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
        ll = (l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]) + l[:, 2] * l[:, 2]
    return d, mm, ll, vis


def associate_depth_views_gated(points_idx, normals_w, K, Kinv, lw_cams, dms, nmaps, scale, center, half, max_dist=0.0, min_cos=0.5):
    """gn_np.associate_depth_views through the gate.  normals_w: the samples' warped normals n'; nmaps: (V, H, W, 3) float32 live
    normal maps.  Returns (corr (S, 3), valid (S,), chosen view (S,), edge (S,)): edge marks the samples for which, in some view
    that passed every other test, the gate's decision lies within EDGE of its threshold (a comparison against the device leaves
    them out)."""
    P = np.asarray(points_idx, dtype=np.float64)
    best = np.full(len(P), np.inf)
    corr = np.zeros_like(P)
    view = np.full(len(P), -1, dtype=np.int64)
    edge = np.zeros(len(P), dtype=bool)
    for v, (lw_cam, dm) in enumerate(zip(lw_cams, dms)):
        lw_cam = np.asarray(lw_cam, dtype=np.float64)
        c, ok = gn_np.associate_depth(P, K, Kinv, lw_cam, dm, scale, center, half)
        dd = c - P
        d2 = dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1] + dd[:, 2] * dd[:, 2]
        if max_dist > 0:
            ok = ok & (d2 <= max_dist * max_dist)
        d, mm, ll, _ = gate_terms(P, normals_w, K, lw_cam, np.asarray(nmaps[v]), scale, center, half)
        with np.errstate(all="ignore"):
            thr = (min_cos * min_cos) * (mm * ll)
            passed = (d > 0) & (d * d >= thr)                       # (a NaN fails both)
            ml = mm * ll
            near = np.isfinite(ml) & (ml > 0) & ((np.abs(d * d - thr) <= EDGE * ml) | (np.abs(d) <= EDGE * np.sqrt(ml)))
        edge |= ok & near
        ok = ok & passed
        take = ok & (d2 < best)
        best = np.where(take, d2, best)
        corr = np.where(take[:, None], c, corr)
        view = np.where(take, v, view)
    return corr, view >= 0, view, edge


def pixels(points_idx, K, lw_cam, H, W, scale, center, half):
    """(ui, vi, inside) of every sample in ONE view: the pixel the association takes its depth and its live normal from."""
    P = np.asarray(points_idx, dtype=np.float64)
    lw_cam = np.asarray(lw_cam, dtype=np.float64)
    cam = (scale * (P - half) + center) @ lw_cam[:, :3].T + lw_cam[:, 3]
    u, v, ok = O.project_to_pixel(K, cam)
    vis = ok & (u >= 0) & (u < W - 1) & (v >= 0) & (v < H - 1)
    return np.where(vis, np.rint(u), 0).astype(np.int64), np.where(vis, np.rint(v), 0).astype(np.int64), vis
