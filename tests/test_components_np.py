"""CPU: tests/components_np.py, the numpy restatement the GPU tests of K23 compare with, against independent statements of the
same things -- a plain breadth-first search, scipy's csgraph as a second opinion, python loops for the area order and the
compaction."""
from collections import deque

import numpy as np
import pytest

import components_np as CN
from components_cases import CASES, KEEP_MASKS, keep_mask


def bfs_roots(n_verts, faces):
    adj = [[] for _ in range(n_verts)]
    for a, b, c in np.asarray(faces).tolist():
        adj[a] += [b, c]
        adj[b] += [a, c]
        adj[c] += [a, b]
    root = np.full(n_verts, -1, dtype=np.int32)
    for s in range(n_verts):                                # ascending: the first vertex to reach a component is its lowest
        if root[s] >= 0:
            continue
        root[s] = s
        todo = deque([s])
        while todo:
            for w in adj[todo.popleft()]:
                if root[w] < 0:
                    root[w] = s
                    todo.append(w)
    return root


@pytest.fixture(scope="module")
def restated():
    return {name: CN.components(v, f) for name, (v, f) in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_labels_equal_a_breadth_first_search(restated, name):
    v, f = CASES[name]
    r = restated[name]
    root = bfs_roots(len(v), f)
    assert np.array_equal(r["vert_root"], root)
    uniq = np.unique(root)
    assert r["n"] == len(uniq) and np.array_equal(r["root"], uniq)
    assert np.array_equal(r["vert_comp"], np.searchsorted(uniq, root))
    assert all(r["vert_comp"][a] == r["vert_comp"][b] == r["vert_comp"][c] == k for (a, b, c), k in zip(f.tolist(), r["face_comp"].tolist()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_labels_equal_scipy(restated, name):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    v, f = CASES[name]
    if len(v) == 0:
        return
    i = np.concatenate([f[:, 0], f[:, 0], f[:, 1]])
    j = np.concatenate([f[:, 1], f[:, 2], f[:, 2]])
    n, lab = connected_components(sp.coo_matrix((np.ones(len(i)), (i, j)), shape=(len(v), len(v))), directed=False)
    r = restated[name]
    assert n == r["n"]
    # the same partition: scipy's labels and ours determine each other
    assert len(set(zip(lab.tolist(), r["vert_comp"].tolist()))) == n


@pytest.mark.parametrize("name", sorted(CASES))
def test_table_equals_python_loops(restated, name):
    v, f = CASES[name]
    r = restated[name]
    C = r["n"]
    areas = CN.face_areas(v, f)
    assert np.array_equal(r["n_verts"], np.bincount(r["vert_comp"], minlength=C))
    assert np.array_equal(r["n_faces"], np.bincount(r["face_comp"], minlength=C))
    assert r["n_verts"].sum() == len(v) and r["n_faces"].sum() == len(f)
    # the area order, spelled out: chunk partials from their first face, then the partials from the first chunk
    partial = {}
    for i, (k, a) in enumerate(zip(r["face_comp"].tolist(), areas.tolist())):
        key = (k, i // 256)
        partial[key] = a if key not in partial else partial[key] + a
    want = {}
    for (k, _), p in sorted(partial.items()):
        want[k] = p if k not in want else want[k] + p
    assert np.array_equal(r["area"], np.array([want.get(k, 0.0) for k in range(C)], dtype=np.float64))
    for k in range(min(C, 50)):
        mine = v[r["vert_comp"] == k]
        assert np.array_equal(r["bbox_min"][k], mine.min(axis=0)) and np.array_equal(r["bbox_max"][k], mine.max(axis=0))


def test_box_keys_order_doubles_and_carry_nan():
    x = np.array([-np.inf, -1.5, -0.0, 0.0, 5e-324, 2.0, np.inf])
    k, nan = CN._keys(x)
    assert np.all(k[1:] > k[:-1]) and not nan.any() and k.min() > 0 and k.max() < CN._ALL
    assert np.array_equal(CN._unkey(k).view(np.uint64), x.view(np.uint64))
    v = np.array([[0.0, 0, 0], [1, np.nan, 0], [0, 1, 0], [5, 5, 5], [6, 5, 5], [5, 6, 5]])
    r = CN.components(v, np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32))
    assert np.isnan(r["bbox_min"][0, 1]) and np.isnan(r["bbox_max"][0, 1]) and np.isnan(r["area"][0])
    assert np.array_equal(r["bbox_min"][0, [0, 2]], [0, 0]) and np.array_equal(r["bbox_max"][0, [0, 2]], [1, 0])
    assert np.array_equal(r["bbox_min"][1], [5, 5, 5]) and r["area"][1] == 0.5


@pytest.mark.parametrize("drop", [True, False])
@pytest.mark.parametrize("kind", KEEP_MASKS)
@pytest.mark.parametrize("name", ["degenerate_duplicate_unreferenced", "isolated_V257", "soup_1025", "no_faces_5_verts", "no_vertices"])
def test_compaction_equals_python_loops(restated, name, kind, drop):
    v, f = CASES[name]
    r = restated[name]
    keep = keep_mask(kind, r["n"])
    kept, vmap, f2 = CN.compact(f, r["vert_comp"], r["face_comp"], keep, drop)
    faces_kept = [row for row, k in zip(f.tolist(), r["face_comp"].tolist()) if keep[k]]
    named = {i for row in faces_kept for i in row}
    want = [i for i in range(len(v)) if keep[r["vert_comp"][i]] and (not drop or i in named)]
    assert kept.tolist() == want
    assert vmap.tolist() == [want.index(i) if i in set(want) else -1 for i in range(len(v))] if len(v) < 100 else True
    assert np.array_equal(kept[vmap[kept]], kept) and (vmap >= 0).sum() == len(kept)
    assert np.array_equal(kept[f2].reshape(-1, 3), np.asarray(faces_kept, dtype=np.int32).reshape(-1, 3))


def test_keep_mask_ranks_by_faces_and_breaks_ties_by_id():
    tab = dict(n_faces=np.array([3, 7, 7, 1, 0]), area=np.array([1.0, 2.0, np.nan, 0.1, 0.0]))
    assert CN.keep_mask(tab, keep_largest=1).tolist() == [False, True, False, False, False]
    assert CN.keep_mask(tab, keep_largest=3).tolist() == [True, True, True, False, False]
    assert CN.keep_mask(tab, min_faces=1).tolist() == [True, True, True, True, False]
    assert CN.keep_mask(tab, min_area=0.5).tolist() == [True, True, True, False, False]
