"""CPU: the numpy restatement of K25 (tests/smooth_np.py) against a plain-Python brute force, bit for bit; the boundary counts
of tests/smooth_cases.py; iters = 0; uniform weights against the dense umbrella matrix; the clamp of an obtuse cotangent; and the
recovery figures of tests/golden/smooth_recovery.json, which the device reproduces through equal bits."""
import json
import math
import os

import numpy as np
import pytest

import smooth_np as SN
from smooth_cases import CASES, CENTRE, CLOSED, FLAGGED, RADIUS, icosphere, noisy_icosphere

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smooth_recovery.json")
SMALL = [n for n in sorted(CASES) if len(CASES[n][0]) <= 60]


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def brute_lists(v, f):
    """Per vertex, its (a, b) pairs in ascending face then corner order, from the faces alone."""
    lists = [[] for _ in range(len(v))]
    for face in f.tolist():
        for c in range(3):
            lists[face[c]].append((face[(c + 1) % 3], face[(c + 2) % 3]))
    return lists


def brute_flag(lists, v):
    ent = [u for pair in lists[v] for u in pair]
    return any(ent.count(u) != 2 for u in ent if u != v)


def brute_weights(p, v, a, b):
    sub = lambda x, y: [x[k] - y[k] for k in range(3)]
    dot = lambda d, g: (d[0] * g[0] + d[1] * g[1]) + d[2] * g[2]
    e1, e2 = sub(p[a], p[v]), sub(p[b], p[v])
    n0, n1, n2 = e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]
    A2 = math.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    if not A2 > 0:
        return 0.0, 0.0
    qa, qb = dot(sub(p[v], p[b]), sub(p[a], p[b])) / A2, dot(sub(p[v], p[a]), sub(p[b], p[a])) / A2
    return (qa if qa > 0 else 0.0), (qb if qb > 0 else 0.0)


def brute_smooth(verts, faces, x, iters, lam, mu, weights, boundary):
    p = np.asarray(verts, dtype=np.float64).tolist()
    lists = brute_lists(p, faces)
    flags = [brute_flag(lists, v) for v in range(len(p))]
    w = [[brute_weights(p, v, a, b) if weights == "cotangent" else (1.0, 1.0) for a, b in lists[v]] for v in range(len(p))]
    x = np.asarray(x, dtype=np.float64)
    K = int(np.prod(x.shape[1:]))
    x = x.reshape(len(p), K).tolist()
    for factor in [fac for _ in range(iters) for fac in ((lam, mu) if mu != 0.0 else (lam,))]:
        new = []
        for v in range(len(p)):
            acc, W = [0.0] * K, 0.0
            for (a, b), (wa, wb) in zip(lists[v], w[v]):
                for k in range(K):
                    acc[k] += wa * (x[a][k] - x[v][k])
                    acc[k] += wb * (x[b][k] - x[v][k])
                W += wa
                W += wb
            if W > 0 and not (boundary == "fixed" and flags[v]):
                new.append([x[v][k] + factor * (acc[k] / W) for k in range(K)])
            else:
                new.append(list(x[v]))
        x = new
    return np.asarray(x, dtype=np.float64).reshape(len(p), K), np.asarray(flags, dtype=bool)


def brute_normals(verts, faces, sign):
    p = np.asarray(verts, dtype=np.float64).tolist()
    out = []
    for v, lst in enumerate(brute_lists(p, faces)):
        s = [0.0, 0.0, 0.0]
        for a, b in lst:
            e1, e2 = [p[a][k] - p[v][k] for k in range(3)], [p[b][k] - p[v][k] for k in range(3)]
            s[0] += e1[1] * e2[2] - e1[2] * e2[1]
            s[1] += e1[2] * e2[0] - e1[0] * e2[2]
            s[2] += e1[0] * e2[1] - e1[1] * e2[0]
        m = [sign * t for t in s]
        length = math.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        out.append([t / length for t in m] if length > 0 else [0.0, 0.0, 0.0])
    return np.asarray(out, dtype=np.float64).reshape(len(p), 3)


@pytest.mark.parametrize("name", SMALL)
def test_the_restatement_equals_a_plain_python_brute_force_bit_for_bit(name):
    v, f = CASES[name]
    attr = np.cos(v * 1.3) + 0.25
    mu = SN.taubin_mu(0.5, 0.1)
    for weights in ("uniform", "cotangent"):
        for boundary in ("fixed", "free"):
            L = SN.Laplacian(v, f, weights, boundary)
            for x in (v, attr[:, :1]):
                for m in (mu, 0.0):
                    want, flags = brute_smooth(v, f, x, 2, 0.5, m, weights, boundary)
                    got = L.smooth(x, iters=2, lam=0.5, mu=m)
                    assert np.array_equal(raw(got), raw(want.reshape(got.shape))), (name, weights, boundary, m)
                    assert np.array_equal(L.boundary, flags)
    for sign in (1.0, -1.0):
        assert np.array_equal(raw(SN.vertex_normals(v, f, sign)), raw(brute_normals(v, f, sign))), (name, sign)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_boundary_rule_flags_what_the_case_says(name):
    v, f = CASES[name]
    L = SN.Laplacian(v, f)
    if FLAGGED[name] is not None:
        assert int(L.boundary.sum()) == FLAGGED[name]
    if name in CLOSED:
        assert not L.boundary.any()


def test_the_flagged_vertices_are_the_ones_the_cases_are_built_for():
    assert (len(icosphere(1)[0]), len(icosphere(3)[0]), len(icosphere(3)[1])) == (42, 642, 1280)
    v, f = CASES["lattice_9x7"]
    i, j = np.divmod(np.arange(63), 7)
    assert np.array_equal(SN.Laplacian(v, f).boundary, (i == 0) | (i == 8) | (j == 0) | (j == 6))
    assert SN.Laplacian(*CASES["three_on_one_edge"]).boundary.all() and SN.Laplacian(*CASES["triangle"]).boundary.all()
    v, f = CASES["face_twice"]
    assert sorted(np.nonzero(SN.Laplacian(v, f).boundary)[0].tolist()) == sorted(f[1].tolist())
    v, f = CASES["isolated_vertices"]
    L = SN.Laplacian(v, f, boundary="free")
    unref = np.setdiff1d(np.arange(len(v)), f.reshape(-1))
    assert len(unref) == 3 and not L.boundary[unref].any()
    assert np.array_equal(raw(L.smooth(iters=3)[unref]), raw(v[unref]))          # never flagged, never moves
    assert np.array_equal(SN.vertex_normals(v, f)[unref], np.zeros((3, 3)))
    v, f = CASES["bipyramid_hub_last"]
    assert SN.Laplacian(v, f).deg[-1] == 300 and len(v) - 1 == f.max()


@pytest.mark.parametrize("name", sorted(CASES))
def test_iters_0_is_the_identity_and_fixed_vertices_keep_their_bits(name):
    v, f = CASES[name]
    for dtype in (np.float64, np.float32):
        x = v.astype(dtype)
        for weights in ("uniform", "cotangent"):
            L = SN.Laplacian(x, f, weights)
            got = L.smooth(iters=0)
            assert got.dtype == dtype and np.array_equal(raw(got), raw(x))
            moved = L.smooth(iters=3)
            assert np.array_equal(raw(moved[L.boundary]), raw(x[L.boundary]))


def test_uniform_weights_on_the_icosphere_are_the_dense_umbrella_operator():
    v, f = CASES["icosphere_1"]
    A = np.zeros((len(v), len(v)))
    for a, b, c in f:
        A[a, b] = A[b, a] = A[b, c] = A[c, b] = A[a, c] = A[c, a] = 1.0
    deg = A.sum(axis=1)
    assert sorted(set(deg.tolist())) == [5.0, 6.0]
    L = SN.Laplacian(v, f)
    assert np.array_equal(L.W, 2.0 * deg)                    # every neighbour twice: once per face on the edge
    want = v + 0.5 * (A @ v / deg[:, None] - v)
    got = L.smooth(iters=1, lam=0.5, mu=0.0)
    assert np.abs(got - want).max() <= 64 * np.finfo(np.float64).eps * np.abs(v).max()
    assert np.abs(got - v).max() > 1e-3                      # (and it moved)


def test_an_obtuse_cotangent_is_clamped_to_0_and_a_zero_area_face_weighs_nothing():
    L = SN.Laplacian(*CASES["obtuse"], weights="cotangent")
    p, v, a, b = L.p, L.v, L.a, L.b
    raw_cot = np.einsum("ij,ij->i", p[v] - p[b], p[a] - p[b])
    assert (raw_cot < 0).any() and (L.wa[raw_cot < 0] == 0).all() and (L.wa >= 0).all() and (L.wb >= 0).all()
    assert (L.W > 0).all()
    C = SN.Laplacian(*CASES["coincident_vertices"], weights="cotangent")
    e1, e2 = C.p[C.a] - C.p[C.v], C.p[C.b] - C.p[C.v]
    flat = ~np.cross(e1, e2).any(axis=1)
    assert flat.sum() >= 6 and (C.wa[flat] == 0).all() and (C.wb[flat] == 0).all()
    assert np.isfinite(C.smooth(iters=3)).all()


def test_taubin_keeps_the_sphere_that_laplace_shrinks():
    """tests/golden/smooth_recovery.json: the figures of the restatement, which tests/test_gpu_smooth.py asserts on the device's
    equal bits.  The bounds are the issue's: ten Taubin iterations at most halve the rms radial deviation (after <= 0.5 before) and
    move the mean radius by at most 0.05; twenty plain Laplacian passes move it by more than 0.5."""
    noisy, f = noisy_icosphere()
    rec = SN.golden_record(noisy, f, CENTRE, RADIUS)
    print(json.dumps(rec, indent=1))
    assert rec["rms_radial_deviation_after_taubin"] <= 0.5 * rec["rms_radial_deviation_before"]
    assert abs(rec["mean_radius_shift_taubin"]) <= 0.05
    assert abs(rec["mean_radius_shift_laplace"]) > 0.5
    assert rec == json.load(open(GOLDEN))
