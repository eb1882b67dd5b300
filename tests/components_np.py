"""numpy restatement of K23 (mesh connected components), output for output as include/dfusion_hip.h defines them: labels, ids,
the per-component table with the stated area order, and the compaction.  Written for the tests: plain, not fast."""
import numpy as np

AREA_CHUNK = 256                       # faces per chunk of the area order
NAN_BITS = np.uint64(0x7FF8000000000000)
_TOP = np.uint64(1) << np.uint64(63)
_ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def labels(n_verts, faces):
    """root (V,) int32: the lowest vertex index of each vertex's component, by repeated minimum propagation over the face
    corners (every vertex takes the lowest label any of its faces holds, until nothing changes)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    root = np.arange(n_verts, dtype=np.int64)
    while len(f):
        m = root[f].min(axis=1)
        new = root.copy()
        for k in range(3):
            np.minimum.at(new, f[:, k], m)
        new = new[new]                                      # (labels are vertex indices: follow them once)
        if np.array_equal(new, root):
            break
        root = new
    return root.astype(np.int32)


def ids(root, faces):
    """(C, comp_root (C,), vert_comp (V,), face_comp (F,)): ids in ascending order of root."""
    root = np.asarray(root, dtype=np.int64)
    comp_root = np.flatnonzero(root == np.arange(len(root)))
    vert_comp = np.searchsorted(comp_root, root).astype(np.int32)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    face_comp = vert_comp[f[:, 0]].astype(np.int32) if len(f) else np.zeros(0, dtype=np.int32)
    return len(comp_root), comp_root.astype(np.int32), vert_comp, face_comp


def _keys(x):
    """The order-preserving key of every double in x, and which of them are NaN."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | _TOP), np.isnan(x)


def _unkey(k):
    b = np.where(k >> np.uint64(63) != 0, k & ~_TOP, ~k)
    return np.where((k == 0) | (k == _ALL), NAN_BITS, b).view(np.float64)


def face_areas(verts, faces):
    """0.5 sqrt(|e1 x e2|^2) per face in fp64, one rounding per operation (numpy contracts nothing)."""
    v = np.asarray(verts).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        a = v[f[:, 0]]
        e1, e2 = v[f[:, 1]] - a, v[f[:, 2]] - a
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def _segment_sums(values, seg_start, seg_len):
    """Per segment, its values added one after the other starting from the first (vectorised over the segments)."""
    out = np.zeros(len(seg_start), dtype=np.float64)
    if len(seg_start) == 0:
        return out
    with np.errstate(all="ignore"):
        out[:] = values[seg_start]
        for k in range(1, int(seg_len.max())):
            m = seg_len > k
            out[m] = out[m] + values[seg_start[m] + k]
    return out


def component_areas(areas, face_comp, n_comp):
    """area[c]: per chunk of 256 faces the component's areas in ascending face index, then the chunks' partials in ascending chunk
    index, each sum starting from its first term; 0.0 without faces."""
    out = np.zeros(n_comp, dtype=np.float64)
    F = len(areas)
    if F == 0:
        return out
    fidx = np.arange(F, dtype=np.int64)
    order = np.lexsort((fidx, face_comp))                   # by component, then face index
    c, j, a = np.asarray(face_comp, dtype=np.int64)[order], (fidx // AREA_CHUNK)[order], areas[order]
    new_seg = np.ones(F, dtype=bool)
    new_seg[1:] = (c[1:] != c[:-1]) | (j[1:] != j[:-1])
    s0 = np.flatnonzero(new_seg)
    partial = _segment_sums(a, s0, np.diff(np.append(s0, F)))
    pc = c[s0]                                              # the partials are in (component, chunk) order already
    new_comp = np.ones(len(s0), dtype=bool)
    new_comp[1:] = pc[1:] != pc[:-1]
    c0 = np.flatnonzero(new_comp)
    out[pc[c0]] = _segment_sums(partial, c0, np.diff(np.append(c0, len(s0))))
    return out


def table(verts, faces, vert_comp, face_comp, n_comp):
    """dict(n_verts, n_faces (int32), bbox_min, bbox_max ((C, 3) float64), area (C,) float64)."""
    v = np.asarray(verts).astype(np.float64).reshape(-1, 3)
    vc = np.asarray(vert_comp, dtype=np.int64)
    n_verts = np.bincount(vc, minlength=n_comp).astype(np.int32)
    n_faces = np.bincount(np.asarray(face_comp, dtype=np.int64), minlength=n_comp).astype(np.int32)
    bmin = np.empty((n_comp, 3), dtype=np.float64)
    bmax = np.empty((n_comp, 3), dtype=np.float64)
    for a in range(3):
        k, nan = _keys(v[:, a])
        lo = np.full(n_comp, _ALL, dtype=np.uint64)
        hi = np.zeros(n_comp, dtype=np.uint64)
        np.minimum.at(lo, vc, np.where(nan, np.uint64(0), k))
        np.maximum.at(hi, vc, np.where(nan, _ALL, k))
        bmin[:, a], bmax[:, a] = _unkey(lo), _unkey(hi)
    area = component_areas(face_areas(v, faces), face_comp, n_comp)
    return dict(n_verts=n_verts, n_faces=n_faces, bbox_min=bmin, bbox_max=bmax, area=area)


def components(verts, faces):
    """Everything mesh.connected_components returns, as a dict of numpy arrays."""
    root = labels(len(verts), faces)
    C, comp_root, vert_comp, face_comp = ids(root, faces)
    out = dict(n=C, vert_root=root, root=comp_root, vert_comp=vert_comp, face_comp=face_comp)
    out.update(table(verts, faces, vert_comp, face_comp, C))
    return out


def compact(faces, vert_comp, face_comp, keep, drop_unreferenced):
    """(kept_vert_idx, vert_map, faces_out)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    keep = np.asarray(keep) != 0
    fk = keep[np.asarray(face_comp, dtype=np.int64)] if len(f) else np.zeros(0, dtype=bool)
    if drop_unreferenced:
        vk = np.zeros(len(vert_comp), dtype=bool)
        vk[f[fk].reshape(-1)] = True
    else:
        vk = keep[np.asarray(vert_comp, dtype=np.int64)] if len(vert_comp) else np.zeros(0, dtype=bool)
    kept = np.flatnonzero(vk).astype(np.int32)
    vmap = np.full(len(vert_comp), -1, dtype=np.int32)
    vmap[kept] = np.arange(len(kept), dtype=np.int32)
    return kept, vmap, vmap[f[fk]].astype(np.int32).reshape(-1, 3)


def keep_mask(tab, min_faces=0, min_area=0.0, keep_largest=None):
    keep = (tab["n_faces"] >= min_faces) & ~(tab["area"] < min_area)
    if keep_largest is not None:
        top = np.zeros(len(keep), dtype=bool)
        top[np.argsort(-tab["n_faces"].astype(np.int64), kind="stable")[:keep_largest]] = True
        keep &= top
    return keep
