"""Exact rational rasterizer: the oracle of tests/test_raster_exact.py and tests/test_gpu_raster_edges.py.

Written from the contract of dfh_render_* in include/dfusion_hip.h in `fractions.Fraction` (integers where a common denominator
allows it); it shares no code with tests/render_np.py, whose expressions restate the kernel's fp64 arithmetic.  Given projected
coordinates as exact rationals it decides coverage, the perspective-correct depth, the float32 rounding of that depth and the
(depth bits, face id) order without a rounding error of its own; only the last step of a result that the contract states in
floating point (a normalisation, a float32 grey level) is done in floating point, and said so below.
"""
import math
from fractions import Fraction as Fr

import numpy as np

SMALL_PIXELS = 64                      # boxes up to this many pixels are walked by one lane (the header documents 64)
# The kernel's fp64 value of 1 / s has about ten roundings behind it, so it differs from the exact value by a few 2^-53
# relative and by no more; 2^-45 is a safe multiple of that, not a measurement.
UNDECIDED_REL = Fr(1, 2 ** 45)
# The bounds the tests hold normals and sample attributes to (derived in the docstring of tests/test_raster_exact.py)
EPS = 2.0 ** -53
SAMPLE_EPS = 12 * EPS
NORMAL_ABS = 2.0 ** -40


def _ceil(q):
    return -((-q.numerator) // q.denominator)


def _floor(q):
    return q.numerator // q.denominator


def _lcm(a, b):
    return a * b // math.gcd(a, b)


def _f32(q):
    """The float32 nearest to the rational q (float() of a Fraction is correctly rounded; where the double rounding could
    matter the pixel is reported as undecided by _near_midpoint)."""
    with np.errstate(over="ignore"):
        return np.float32(float(q))


def _near_midpoint(q, zf):
    """True if the exact depth q lies within relative UNDECIDED_REL of the midpoint between zf = _f32(q) and its float32
    neighbour on q's side."""
    exact = Fr(float(zf))
    if q == exact:
        return False
    other = np.nextafter(zf, np.float32(np.inf) if q > exact else np.float32(-np.inf))
    mid = (exact + Fr(float(other))) / 2
    return abs(q - mid) <= UNDECIDED_REL * q


class Exact:
    """One view's result.  depth (H, W) float32 = -z, 0 where empty; face (H, W) int32, -1 where empty; n_large: (face, view)
    pairs whose clamped box exceeds SMALL_PIXELS (large: their faces); undecided: [(y, x)] (see
    render_exact); a: {(y, x): (a0, a1, a2)} the winner's exact lambda_i / z_i."""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.depth = np.zeros((H, W), dtype=np.float32)
        self.face = np.full((H, W), -1, dtype=np.int32)
        self.n_large = 0
        self.large = []
        self.undecided = []
        self.a = {}

    def pixels(self):
        """Covered pixels in row-major order."""
        return sorted(self.a)


def render_exact(u, v, z, faces, H, W, znear):
    """u, v, z: per-vertex projected coordinates of ONE view as Fractions (None: not finite).  Returns an Exact.
    A pixel is UNDECIDED, and reported as such, if its winner's exact depth lies within relative 2^-45 of a float32 rounding
    midpoint, or if two of its candidates' exact depths differ by less than that without being equal: there the kernel's
    rounding errors could decide, and the oracle does not claim to know the answer."""
    n = len(u)
    znear = Fr(znear)
    out = Exact(H, W)
    cand = {}
    for f, idx in enumerate(faces):
        idx = [int(i) for i in idx]
        if any(i < 0 or i >= n for i in idx):
            continue
        if any(u[i] is None or v[i] is None or z[i] is None for i in idx):
            continue
        U, V, Z = [u[i] for i in idx], [v[i] for i in idx], [z[i] for i in idx]
        if any(zi <= znear for zi in Z):
            continue
        A = (U[2] - U[0]) * (V[1] - V[0]) - (V[2] - V[0]) * (U[1] - U[0])      # E01 at vertex 2
        if A == 0:
            continue
        x0, x1 = max(0, _ceil(min(U))), min(W - 1, _floor(max(U)))
        y0, y1 = max(0, _ceil(min(V))), min(H - 1, _floor(max(V)))
        if x0 > x1 or y0 > y1:
            continue
        if (x1 - x0 + 1) * (y1 - y0 + 1) > SMALL_PIXELS:
            out.n_large += 1
            out.large.append(f)
        # E_ab(x, y) = x (vb - va) - y (ub - ua) + (va (ub - ua) - ua (vb - va)), brought to one integer denominator
        co = []
        for a, b in ((1, 2), (2, 0), (0, 1)):
            du, dv = U[b] - U[a], V[b] - V[a]
            co.append((dv, -du, V[a] * du - U[a] * dv))
        den = A.denominator
        for c in co:
            for t in c:
                den = _lcm(den, t.denominator)
        ico = [tuple(int(t * den) for t in c) for c in co]
        iA = int(A * den)
        sgn = 1 if iA > 0 else -1
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                e = [cx * x + cy * y + c0 for cx, cy, c0 in ico]
                if sgn * e[0] < 0 or sgn * e[1] < 0 or sgn * e[2] < 0:     # the closed triangle: zero counts as inside
                    continue
                a = tuple(Fr(e[i], iA) / Z[i] for i in range(3))
                s = a[0] + a[1] + a[2]
                if s <= 0:
                    continue
                cand.setdefault((y, x), []).append((1 / s, f, a))
    for (y, x), cs in cand.items():
        keyed = []
        for d, f, a in cs:
            zf = _f32(d)
            if np.isfinite(zf):
                keyed.append((int(zf.view(np.uint32)), f, d, a, zf))
        if not keyed:
            continue
        bits, f, d, a, zf = min(keyed, key=lambda k: (k[0], k[1]))
        out.depth[y, x] = -zf
        out.face[y, x] = f
        out.a[(y, x)] = a
        ds = sorted(k[2] for k in keyed)
        if _near_midpoint(d, zf) or any(0 < q - p < UNDECIDED_REL * q for p, q in zip(ds, ds[1:])):
            out.undecided.append((y, x))
    return out


def vertex_ids(res, faces, znear_img, zfar_img):
    """(vid (H, W) int32, grey (H, W) uint8) of dfh_render_vertex_ids from the winner's exact a_i; the grey level in the
    float32 arithmetic the header states."""
    vid = np.full((res.H, res.W), -1, dtype=np.int32)
    grey = np.zeros((res.H, res.W), dtype=np.uint8)
    zf, zn = np.float32(zfar_img), np.float32(znear_img)
    for (y, x), (a0, a1, a2) in res.a.items():
        d = np.float32(-res.depth[y, x])
        if not (float(d) >= znear_img and float(d) <= zfar_img):
            continue
        corner = 0 if (a0 > a1 and a0 > a2) else (1 if a1 > a2 else 2)
        vid[y, x] = int(faces[int(res.face[y, x])][corner])
        g = np.float32(np.float32(np.float32(zf - d) / np.float32(zf - zn)) * np.float32(255))
        grey[y, x] = min(255, max(0, int(g)))                                   # int() truncates toward zero
    return vid, grey


def _unit(m):
    """m / |m| of an exact vector: the squared ratio is exact, its square root is taken in fp64 (error within one ulp)."""
    l2 = m[0] * m[0] + m[1] * m[1] + m[2] * m[2]
    if l2 == 0:
        return [0.0, 0.0, 0.0]
    return [math.copysign(math.sqrt(float(c * c / l2)), float(c)) for c in m]


def camera_normals(res, faces, normals, lw):
    """(H, W, 3) float32: m = a0 n0 + a1 n1 + a2 n2 rotated by R of lw = [R | t], exactly, then normalised in fp64."""
    N = [[Fr(float(c)) for c in row] for row in np.asarray(normals, dtype=np.float64)]
    R = [[Fr(float(lw[i][j])) for j in range(3)] for i in range(3)]
    out = np.zeros((res.H, res.W, 3), dtype=np.float32)
    for (y, x), a in res.a.items():
        idx = faces[int(res.face[y, x])]
        m = [sum(a[i] * N[int(idx[i])][c] for i in range(3)) for c in range(3)]
        out[y, x] = _unit([sum(R[r][c] * m[c] for c in range(3)) for r in range(3)])
    return out


def interpolate(res, faces, attr, unit=False):
    """Perspective-correct interpolation (b_i = a_i / sum a) of the per-vertex rows `attr` at every covered pixel, in row-major
    pixel order: (values (n, 3) float64 -- exact, rounded once -- and, with unit=True, normalised as _unit does; the exact
    length of the unnormalised vector as float64 (n,))."""
    P = [[Fr(float(c)) for c in row] for row in np.asarray(attr, dtype=np.float64)]
    vals, lens = [], []
    for yx in res.pixels():
        a = res.a[yx]
        s = a[0] + a[1] + a[2]
        idx = faces[int(res.face[yx])]
        m = [sum(a[i] / s * P[int(idx[i])][c] for i in range(3)) for c in range(3)]
        lens.append(math.sqrt(float(m[0] * m[0] + m[1] * m[1] + m[2] * m[2])))
        vals.append(_unit(m) if unit else [float(c) for c in m])
    return np.array(vals, dtype=np.float64).reshape(-1, 3), np.array(lens, dtype=np.float64)


def coverage_exact_on_doubles(u, v, faces, H, W):
    """Exact coverage decided on projected DOUBLES (non-dyadic scenes: u, v from render_np.project, each converted to a
    Fraction exactly).  Returns {(y, x): [(face, inside, [(exact edge value, rounding bound of its fp64 expression)] * 3)]} over
    the pixels of every face's clamped box; `inside` is the closed-triangle test.  The bound is
    4 * 2^-53 * (|x - u_a| |v_b - v_a| + |y - v_a| |u_b - u_a|) with (u_a, v_a) the end point the header evaluates from."""
    u = [Fr(float(t)) if np.isfinite(t) else None for t in u]
    v = [Fr(float(t)) if np.isfinite(t) else None for t in v]
    eps4 = Fr(4, 2 ** 53)
    out = {}
    for f, idx in enumerate(faces):
        idx = [int(i) for i in idx]
        if any(i < 0 or i >= len(u) or u[i] is None or v[i] is None for i in idx):
            continue
        U, V = [u[i] for i in idx], [v[i] for i in idx]
        A = (U[2] - U[0]) * (V[1] - V[0]) - (V[2] - V[0]) * (U[1] - U[0])
        if A == 0:
            continue
        x0, x1 = max(0, _ceil(min(U))), min(W - 1, _floor(max(U)))
        y0, y1 = max(0, _ceil(min(V))), min(H - 1, _floor(max(V)))
        sgn = 1 if A > 0 else -1
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                es = []
                for a, b in ((1, 2), (2, 0), (0, 1)):
                    e = (x - U[a]) * (V[b] - V[a]) - (y - V[a]) * (U[b] - U[a])
                    if (U[b], V[b]) < (U[a], V[a]):
                        a, b = b, a
                    bound = eps4 * (abs(x - U[a]) * abs(V[b] - V[a]) + abs(y - V[a]) * abs(U[b] - U[a]))
                    es.append((e, bound))
                inside = all(sgn * e >= 0 for e, _ in es)
                out.setdefault((y, x), []).append((f, inside, es))
    return out


class SceneOracle:
    """Everything the tests compare, for one scene of tests/raster_cases.py (the first 16 views for the maps and samples, every
    view for the vertex ids): depth / face (V, H, W), normal (V, H, W, 3) float32, large = the listed (face, view) pairs as
    [(view, face)], undecided = [(view, y, x)], vid / grey (all views, H, W), and the samples at stride 1: pixel (n,) int64,
    pos / nrm (n, 3) float64, nrm_len (n,) the length of the interpolated normal before it is normalised."""


def render_scene(s, max_views=16):
    o = SceneOracle()
    views = []
    for vi in range(len(s.views)):
        U, V, Z = s.exact[vi]
        views.append(render_exact(U, V, Z, s.faces, s.H, s.W, s.znear))
    first = views[:max_views]
    o.depth = np.stack([r.depth for r in first])
    o.face = np.stack([r.face for r in first])
    o.large = [(vi, f) for vi, r in enumerate(first) for f in r.large]
    o.undecided = [(vi, y, x) for vi, r in enumerate(views) for y, x in r.undecided]
    o.normal = np.stack([camera_normals(r, s.faces, s.normals, s.views[vi].lw()) for vi, r in enumerate(first)])
    ids = [vertex_ids(r, s.faces, *s.img) for r in views]
    o.vid, o.grey = np.stack([i[0] for i in ids]), np.stack([i[1] for i in ids])
    pix, pos, nrm, ln = [], [], [], []
    for vi, r in enumerate(first):
        pix += [(vi * s.H + y) * s.W + x for y, x in r.pixels()]
        pos.append(interpolate(r, s.faces, s.cpos)[0])
        n, l = interpolate(r, s.faces, s.cnrm, unit=True)
        nrm.append(n), ln.append(l)
    o.pixel = np.array(pix, dtype=np.int64)
    o.pos, o.nrm, o.nrm_len = np.concatenate(pos), np.concatenate(nrm), np.concatenate(ln)
    for a in vars(o).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return o


def normal_excess(got, ref):
    """max over the components of |got - ref| / allowance, allowance = max(2 float32 ulp of ref, 2^-40): <= 1 passes."""
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    allow = np.maximum(2 * np.spacing(np.abs(ref)).astype(np.float64), NORMAL_ABS)
    return float((np.abs(got.astype(np.float64) - ref.astype(np.float64)) / allow).max()) if got.size else 0.0


def sample_bounds(s, o):
    """(bound on |pos - oracle|, per-sample bounds on |nrm - oracle| (n, 1)) for scene s and its SceneOracle o."""
    bp = SAMPLE_EPS * np.abs(s.cpos).max()
    with np.errstate(divide="ignore"):
        bn = 3 * SAMPLE_EPS * np.abs(s.cnrm).max() / o.nrm_len + 4 * EPS
    return bp, bn[:, None]
