"""CPU: the numpy restatement of K24 (tests/simplify_np.py) against an independent brute force in plain Python (dicts, loops and
Python floats, which are fp64 with one rounding per operation), its structural properties on every case of
tests/simplify_cases.py, and the recorded figures of tests/golden/simplify_recovery.json (tools/make_simplify_golden.py)."""
import json
import math
import os

import numpy as np
import pytest

import simplify_np as SN
from simplify_cases import CASES, ONE_VERTEX_A_CELL, REG_CASES, cube_side, sphere

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simplify_recovery.json")
MODES = ("quadric", "mean")


def brute_force(verts, faces, cell, origin, mode, reg, drop_unreferenced=True):
    """The definition of include/dfusion_hip.h once more, one scalar at a time."""
    P = [[float(x) for x in row] for row in np.asarray(verts, dtype=np.float64)]
    Fs = [[int(i) for i in row] for row in faces]
    V = len(P)
    cell = float(cell)
    if origin is None:
        origin = [min(p[a] for p in P) for a in range(3)] if V else [0.0, 0.0, 0.0]
    origin = [float(o) for o in origin]
    keys, ctrs = [], []
    for p in P:
        c = [math.floor((p[a] - origin[a]) / cell) for a in range(3)]
        assert all(0 <= x < (1 << 21) for x in c)
        keys.append((c[0] << 42) + (c[1] << 21) + c[2])
        ctrs.append([origin[a] + (c[a] + 0.5) * cell for a in range(3)])
    ids, members = {}, []
    for v, k in enumerate(keys):                             # ascending v: a new key is a new cluster, numbered by its lowest vertex
        if k not in ids:
            ids[k] = len(members)
            members.append([])
        members[ids[k]].append(v)
    vc = [ids[k] for k in keys]
    Qv = [[0.0] * 10 for _ in range(V)]
    if mode == "quadric":
        for f in Fs:                                         # ascending face, then corner
            a, b, c = (P[i] for i in f)
            e1 = [b[i] - a[i] for i in range(3)]
            e2 = [c[i] - a[i] for i in range(3)]
            n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            for v in f:
                q = [a[i] - ctrs[v][i] for i in range(3)]
                d = -((n[0] * q[0] + n[1] * q[1]) + n[2] * q[2])
                ten = [n[0] * n[0], n[0] * n[1], n[0] * n[2], n[1] * n[1], n[1] * n[2], n[2] * n[2], d * n[0], d * n[1], d * n[2], d * d]
                for k in range(10):
                    Qv[v][k] += ten[k]
    out, fell = [], 0
    for mem in members:
        ctr = ctrs[mem[0]]
        S, Q = [0.0] * 3, [0.0] * 10
        for v in mem:
            for a in range(3):
                S[a] += P[v][a] - ctr[a]
            for k in range(10):
                Q[k] += Qv[v][k]
        m = [S[a] / float(len(mem)) for a in range(3)]
        x = m
        if mode == "quadric":
            x = solve(Q, m, cell, float(reg))
            if x is None:
                x, fell = m, fell + 1
        out.append([ctr[a] + x[a] for a in range(3)])
    seen, new_faces, face_idx = set(), [], []
    for i, f in enumerate(Fs):
        t = [vc[v] for v in f]
        if t[0] == t[1] or t[1] == t[2] or t[0] == t[2] or tuple(sorted(t)) in seen:
            continue
        seen.add(tuple(sorted(t)))
        new_faces.append(t)
        face_idx.append(i)
    used = sorted({c for t in new_faces for c in t}) if drop_unreferenced else list(range(len(members)))
    cmap = {c: i for i, c in enumerate(used)}
    return dict(verts=[out[c] for c in used], faces=[[cmap[c] for c in t] for t in new_faces], face_idx=face_idx,
                vert_map=[cmap.get(c, -1) for c in vc], vert_cluster=vc, n_clusters=len(members), n_fallback=fell)


def solve(Q, m, cell, reg):
    t = (Q[0] + Q[3]) + Q[5]
    if not t > 0:
        return None
    lam = reg * t
    M00, M10, M20, M11, M21, M22 = Q[0] + lam, Q[1], Q[2], Q[3] + lam, Q[4], Q[5] + lam
    r = [lam * m[a] - Q[6 + a] for a in range(3)]
    d0 = M00
    if not d0 > 0:
        return None
    l10, l20 = M10 / d0, M20 / d0
    d1 = M11 - l10 * M10
    if not d1 > 0:
        return None
    t21 = M21 - l20 * M10
    l21 = t21 / d1
    d2 = (M22 - l20 * M20) - l21 * t21
    if not d2 > 0:
        return None
    y0 = r[0]
    y1 = r[1] - l10 * y0
    y2 = (r[2] - l20 * y0) - l21 * y1
    x2 = y2 / d2
    x1 = y1 / d1 - l21 * x2
    x0 = (y0 / d0 - l10 * x1) - l20 * x2
    half = 0.5 * cell
    if not (abs(x0) <= half and abs(x1) <= half and abs(x2) <= half):
        return None
    return [x0, x1, x2]


def runs(name):
    return [(mode, reg) for mode in MODES for reg in ((1e-3, 0.0) if name in REG_CASES and mode == "quadric" else (1e-3,))]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3).view(np.uint64)


@pytest.mark.parametrize("drop", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_restatement_equals_the_brute_force(name, drop):
    v, f, cell, origin = CASES[name]
    for mode, reg in runs(name):
        got = SN.simplify(v, f, cell=cell, origin=origin, mode=mode, reg=reg, drop_unreferenced=drop)
        want = brute_force(v, f, cell, origin, mode, reg, drop)
        what = (name, mode, reg)
        assert got["vert_cluster"].tolist() == want["vert_cluster"], what
        assert got["faces"].tolist() == want["faces"] and got["face_idx"].tolist() == want["face_idx"], what
        assert got["vert_map"].tolist() == want["vert_map"], what
        assert (got["n_clusters"], got["n_fallback"]) == (want["n_clusters"], want["n_fallback"]), what
        assert np.array_equal(bits(got["verts"]), bits(want["verts"])), what


@pytest.mark.parametrize("name", sorted(CASES))
def test_properties(name):
    v, f, cell, origin = CASES[name]
    for mode, reg in runs(name):
        r = SN.simplify(v, f, cell=cell, origin=origin, mode=mode, reg=reg)
        nf = r["faces"].astype(np.int64)
        assert ((nf[:, 0] != nf[:, 1]) & (nf[:, 1] != nf[:, 2]) & (nf[:, 0] != nf[:, 2])).all()
        assert len(np.unique(np.sort(nf, axis=1), axis=0)) == len(nf)
        assert (np.diff(r["face_idx"]) > 0).all()
        assert len(nf) == 0 or (nf.min() >= 0 and nf.max() < len(r["verts"]))
        if len(v):                                           # inside its cell: cell / 2 an axis from the centre, plus the last rounding
            o = np.min(v, axis=0) if origin is None else np.asarray(origin, dtype=np.float64)
            _, _, ctr = SN.cells(v, cell, o)
            cctr = np.zeros((r["n_clusters"], 3))
            cctr[r["vert_cluster"]] = ctr
            slack = np.spacing(np.abs(cctr) + 0.5 * cell)
            assert (np.abs(r["cluster_verts"] - cctr) <= 0.5 * cell + slack).all()
        full = SN.simplify(v, f, cell=cell, origin=origin, mode=mode, reg=reg, drop_unreferenced=False)
        assert len(full["verts"]) == full["n_clusters"] and (full["vert_map"] == full["vert_cluster"]).all()
        assert np.array_equal(full["face_idx"], r["face_idx"])


@pytest.mark.parametrize("name", ONE_VERTEX_A_CELL)
def test_one_vertex_a_cell_keeps_the_input_faces_and_ids(name):
    v, f, cell, origin = CASES[name]
    r = SN.simplify(v, f, cell=cell, origin=origin, drop_unreferenced=False)
    assert r["n_clusters"] == len(v) and r["vert_cluster"].tolist() == list(range(len(v)))
    seen, want = set(), []
    for t in f.tolist():
        if len(set(t)) == 3 and tuple(sorted(t)) not in seen:
            seen.add(tuple(sorted(t)))
            want.append(t)
    assert r["faces"].tolist() == want
    if name == "duplicate_faces":
        assert len(want) < len(f)


def test_a_vertex_permutation_keeps_the_membership_and_numbers_by_lowest_index():
    from simplify_cases import cube, permuted
    v, f = cube()
    pv, pf, perm = permuted(v, f)
    a = SN.simplify(v, f, cell=3.0)
    b = SN.simplify(pv, pf, cell=3.0)
    assert a["n_clusters"] == b["n_clusters"] and len(a["faces"]) == len(b["faces"])
    group = lambda vc, ident: sorted(sorted(ident[np.nonzero(vc == c)[0]].tolist()) for c in range(vc.max() + 1))
    assert group(a["vert_cluster"], np.arange(len(v))) == group(b["vert_cluster"], perm)
    firsts = [np.nonzero(b["vert_cluster"] == c)[0].min() for c in range(b["n_clusters"])]
    assert firsts == sorted(firsts)


def test_attributes_average_in_fp64_and_keep_their_dtype():
    v, f, cell, origin = CASES["cube"]
    a32 = (v[:, :2] * 0.37).astype(np.float32)
    a64 = v[:, 0] * 1.7
    r = SN.simplify(v, f, (a32, a64), cell=cell, drop_unreferenced=False)
    assert r["attrs"][0].dtype == np.float32 and r["attrs"][0].shape == (r["n_clusters"], 2) and r["attrs"][1].dtype == np.float64
    for c in (0, 7, r["n_clusters"] - 1):
        mem = np.nonzero(r["vert_cluster"] == c)[0]
        s = 0.0
        for i in mem:
            s += float(a64[i])
        assert r["attrs"][1][c] == s / float(len(mem))


def test_the_restatement_refuses_what_the_device_refuses():
    v, f, cell, origin = CASES["triangle_three_cells"]
    bad = v.copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError):
        SN.simplify(bad, f, cell=cell, origin=origin)
    with pytest.raises(ValueError):
        SN.simplify(v, f, cell=1e-7, origin=origin)
    with pytest.raises(ValueError):
        SN.simplify(v, np.array([[0, 1, 3]]), cell=cell, origin=origin)


def test_reg_0_on_the_plane_falls_back_through_the_pivot_test():
    v, f, cell, origin = CASES["plane"]
    r = SN.simplify(v, f, cell=cell, origin=origin, reg=0.0, drop_unreferenced=False)
    assert r["n_fallback"] == r["n_clusters"] > 0            # normal (0, 0, n): A00 = 0, the first pivot is not above 0
    m = SN.simplify(v, f, cell=cell, origin=origin, mode="mean", drop_unreferenced=False)
    assert np.array_equal(bits(r["verts"]), bits(m["verts"]))
    assert SN.simplify(v, f, cell=cell, origin=origin, reg=1e-3)["n_fallback"] == 0


def sphere_case():
    sv, sf = sphere()
    return sv, sf, 2.0, (12.3, 12.1, 11.7), 10.0


def test_the_restatement_reproduces_the_golden():
    want = json.load(open(GOLDEN))
    got = SN.golden_record(CASES, REG_CASES, cube_side(), sphere_case())
    assert got["counts"] == want["counts"]
    for shape in ("cube", "sphere"):
        for mode in MODES:
            for k, x in want[shape][mode].items():
                assert got[shape][mode][k] == pytest.approx(x, rel=1e-9, abs=1e-12), (shape, mode, k)


def test_the_quadric_representative_recovers_the_cube_corners():
    want = json.load(open(GOLDEN))["cube"]
    v, f, cell, origin = CASES["cube"]
    q = SN.cube_measures(SN.simplify(v, f, cell=cell, mode="quadric")["verts"], *cube_side())
    m = SN.cube_measures(SN.simplify(v, f, cell=cell, mode="mean")["verts"], *cube_side())
    print("corner distance: quadric %.6f, mean %.6f; mean surface error: quadric %.6f, mean %.6f"
          % (q["corner_distance_max"], m["corner_distance_max"], q["surface_error_mean"], m["surface_error_mean"]))
    assert q["corner_distance_max"] < 0.1 * m["corner_distance_max"]
    assert want["quadric"]["corner_distance_max"] < 0.1 * want["mean"]["corner_distance_max"]
