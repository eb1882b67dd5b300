"""CPU: the rasterizer's numpy restatement (tests/render_np.py, render_samples_np.py, pool_np.py) against the exact rational
oracle (tests/raster_exact.py) on the scenes of tests/raster_cases.py.

The restatement repeats the kernel's fp64 expressions, so it can only show that the device runs that arithmetic; the oracle
is written from the contract in include/dfusion_hip.h and decides coverage, depth and order without rounding.  This file ties
the two together without a device (tests/test_gpu_raster_edges.py ties the kernel to the oracle): on every scene the projection
is exact, no pixel is undecided, depth bits / face ids / listed pairs / vertex ids / grey levels / sample pixels are equal,
and normals and sample attributes are within the bounds derived below.  A table of mutations of the restatement, each of which
at least one named scene must catch, shows that the scenes bite.

Bounds.  NORMAL: a rendered normal component is within 2 float32 ulp of the oracle's (the bar of tests/test_gpu_render.py) or
within 2^-40 absolute (the fp64 error budget of a unit vector's component that is nearly zero, where a float32 ulp is
meaningless).  SAMPLE: in these scenes the edge values e_i and the area A are exact in fp64 (quarter-pixel grid), so with
eps = 2^-53: lambda_i = e_i / A and a_i = lambda_i / z_i carry at most 2 eps, s = (a0 + a1) + a2 of non-negative terms at most
2 + 2 = 4 eps, b_i = a_i / s at most 2 + 4 + 1 = 7 eps, each product b_i P_i 8 eps, the two additions 2 eps more:
|pos - exact| <= 10 eps sum_i b_i |P_i| <= 10 eps max|P| as the b_i are non-negative and sum to 1; with the oracle's own final
rounding and second-order terms, SAMPLE_EPS = 12 eps.  The interpolated normal m has the same bound delta = 12 eps max|N| per
component, so |dm| <= sqrt(3) delta; a component of m / |m| moves by at most delta / |m| from its numerator and sqrt(3) delta / |m|
from the length, under 3 delta / |m|, plus 4 eps for the square root, the division and the oracle's own two roundings.  The restatement's measured deviation is printed by test_samples_restatement_within_bound (DESIGN.md quotes it).
"""
import functools

import numpy as np
import pytest

import pool_np as PN
import raster_cases as RC
import raster_exact as RX
import render_np as R
import render_samples_np as RS

EPS, SAMPLE_EPS = RX.EPS, RX.SAMPLE_EPS
oracle, normal_excess, sample_bounds = RC.oracle, RX.normal_excess, RX.sample_bounds


# ---- the restatement of a whole scene (under whatever mutation is in force) ---------------------------------------------------
def render_keyed(s, vi, mode):
    """A local variant of render_np.render for one view, built on render_np.raster_triangle: mode "f32" is the contract (the
    key is the float32 depth, then the face id), "f64" orders on the fp64 depth instead, "higher_id" sends ties to the higher
    face id.  Returns (depth, face)."""
    vw = s.views[vi]
    with np.errstate(all="ignore"):
        U, V, Z = R.project(s.verts, vw.K(), vw.lw(), **s.geom)
    best = {}
    for f, idx in enumerate(s.faces.astype(np.int64)):
        if idx.min() < 0 or idx.max() >= len(s.verts):
            continue
        r = R.raster_triangle(U[idx], V[idx], Z[idx], s.H, s.W, s.znear)
        if r is None:
            continue
        x0, y0, ok, z64, zf = r
        for j, i in zip(*np.nonzero(ok)):
            d32 = int(zf[j, i].view(np.uint32))
            key = {"f32": (d32, f), "f64": (float(z64[j, i]), f), "higher_id": (d32, -f)}[mode]
            if (y0 + j, x0 + i) not in best or key < best[(y0 + j, x0 + i)][0]:
                best[(y0 + j, x0 + i)] = (key, zf[j, i], f)
    depth, face = np.zeros((s.H, s.W), dtype=np.float32), np.full((s.H, s.W), -1, dtype=np.int32)
    for (y, x), (_, zf, f) in best.items():
        depth[y, x], face[y, x] = -zf, f
    return depth, face


def listed_pairs(s, n_views, unclamped=False):
    """The small kernel's switch restated on render_np.setup: [(view, face)] whose clamped box exceeds 64 pixels.
    unclamped=True is the mutation that sizes the box before the clamp."""
    out = []
    for vi in range(n_views):
        vw = s.views[vi]
        with np.errstate(all="ignore"):
            U, V, Z = R.project(s.verts, vw.K(), vw.lw(), **s.geom)
        for f, idx in enumerate(s.faces.astype(np.int64)):
            if idx.min() < 0 or idx.max() >= len(s.verts):
                continue
            st = R.setup(U[idx], V[idx], Z[idx], s.H, s.W, s.znear)
            if st is None:
                continue
            _, x0, x1, y0, y1 = st
            if unclamped:
                x0, x1 = int(np.ceil(U[idx].min())), int(np.floor(U[idx].max()))
                y0, y1 = int(np.ceil(V[idx].min())), int(np.floor(V[idx].max()))
            if (x1 - x0 + 1) * (y1 - y0 + 1) > RX.SMALL_PIXELS:
                out.append((vi, f))
    return out


def restate(s, key="f32", unclamped=False, img=None):
    """The restatement's maps of a scene: dict(depth, face, listed, vid, grey)."""
    nv = min(len(s.views), RC.RENDER_MAX_VIEWS)
    if key == "f32":
        maps = [R.render(s.verts, s.faces, None, s.views[vi].K(), s.views[vi].lw(), s.H, s.W, znear=s.znear, **s.geom) for vi in range(nv)]
        depth, face = np.stack([m[0][0] for m in maps]), np.stack([m[2][0] for m in maps])
    else:
        maps = [render_keyed(s, vi, key) for vi in range(nv)]
        depth, face = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    zn, zf = s.img if img is None else img
    vid, grey = PN.vertex_ids(s.verts, s.faces, s.Ks(), s.lws(), s.H, s.W, zn, zf, znear=s.znear, **s.geom)
    return dict(depth=depth, face=face, listed=listed_pairs(s, nv, unclamped), vid=vid, grey=grey)


def differences(s, got):
    """What of `got` (restate's dict) differs from the oracle, as strings; empty when all is equal."""
    o = oracle(s.name)
    out = []
    if not np.array_equal(got["face"], o.face):
        vi, y, x = np.argwhere(got["face"] != o.face)[0]
        out.append("face map: %d pixels, first view %d (%d, %d): %d, oracle %d" % ((got["face"] != o.face).sum(), vi, x, y, got["face"][vi, y, x],
                                                                                   o.face[vi, y, x]))
    db = got["depth"].view(np.uint32) != o.depth.view(np.uint32)
    if db.any():
        vi, y, x = np.argwhere(db)[0]
        out.append("depth bits: %d pixels, first view %d (%d, %d): %r, oracle %r" % (db.sum(), vi, x, y, got["depth"][vi, y, x], o.depth[vi, y, x]))
    if sorted(got["listed"]) != sorted(o.large):
        out.append("listed pairs: %d, oracle %d" % (len(got["listed"]), len(o.large)))
    for k, ref in (("vid", o.vid), ("grey", o.grey)):
        if not np.array_equal(got[k], ref):
            vi, y, x = np.argwhere(got[k] != ref)[0]
            out.append("%s: %d pixels, first view %d (%d, %d): %d, oracle %d" % (k, (got[k] != ref).sum(), vi, x, y, got[k][vi, y, x], ref[vi, y, x]))
    return out


# ---- every scene ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.NAMES)
def test_projection_is_exact(name):
    """render_np.project (the kernel's fp64 expressions) gives the intended rationals bit for bit; a vertex that is not finite
    fails the set-up's test in every view."""
    s = RC.scene(name)
    for vi, vw in enumerate(s.views):
        with np.errstate(all="ignore"):
            U, V, Z = R.project(s.verts, vw.K(), vw.lw(), **s.geom)
        eu, ev, ez = s.exact[vi]
        for i in range(len(U)):
            if eu[i] is None:
                assert not (Z[i] > s.znear and np.isfinite(U[i]) and np.isfinite(V[i]))
            else:
                assert (RX.Fr(float(U[i])), RX.Fr(float(V[i])), RX.Fr(float(Z[i]))) == (eu[i], ev[i], ez[i]), (name, vi, i)


@pytest.mark.parametrize("name", RC.NAMES)
def test_restatement_equals_oracle(name):
    s, o = RC.scene(name), oracle(name)
    assert o.undecided == [], "%d undecided pixels" % len(o.undecided)
    assert differences(s, restate(s)) == []
    nv = o.depth.shape[0]
    with np.errstate(all="ignore"):                      # (vertices that are not finite)
        normal = np.concatenate([R.render(s.verts, s.faces, s.normals, s.views[vi].K(), s.views[vi].lw(), s.H, s.W, znear=s.znear,
                                          **s.geom)[1] for vi in range(nv)])
    ex = normal_excess(normal, o.normal)
    print("%s: %d covered pixels, %d listed pairs, normal deviation %.3g of the allowance" % (name, (o.face >= 0).sum(), len(o.large), ex))
    assert ex <= 1.0
    assert np.array_equal(normal[o.face < 0], np.zeros_like(normal[o.face < 0]))


@functools.lru_cache(maxsize=None)
def restated_samples(name):
    s, o = RC.scene(name), oracle(name)
    pos, nrm, pix = [], [], []
    for vi in range(o.depth.shape[0]):
        p, n, x = RS.render_samples(s.verts, s.faces, s.cpos, s.cnrm, s.views[vi].K(), s.views[vi].lw(), s.H, s.W, znear=s.znear, **s.geom)
        pos.append(p), nrm.append(n), pix.append(x + vi * s.H * s.W)
    return np.concatenate(pos), np.concatenate(nrm), np.concatenate(pix)


@pytest.mark.parametrize("name", RC.NAMES)
def test_samples_restatement_within_bound(name):
    s, o = RC.scene(name), oracle(name)
    pos, nrm, pix = restated_samples(name)
    assert np.array_equal(pix, o.pixel)
    bp, bn = sample_bounds(s, o)
    dp = np.abs(pos - o.pos).max() if len(pix) else 0.0
    dn = (np.abs(nrm - o.nrm) / bn).max() if len(pix) else 0.0
    print("%s: %d samples, |pos - oracle| max %.3g = %.2f eps max|P| (bound %g eps), normals at %.3g of their bound"
          % (name, len(pix), dp, dp / (EPS * np.abs(s.cpos).max()), SAMPLE_EPS / EPS, dn))
    assert dp <= bp and dn <= 1.0


# ---- the scenes hold what their names say (on the oracle's results) ---------------------------------------------------------------
def test_switch_scenes_sit_on_both_sides_of_64():
    o = oracle("switch_boxes")
    assert [f for v, f in o.large if v == 0] == [2, 3, 4, 5, 9, 12]       # 5x13, 9x8, the two 9x8 twins, the two clamped to 72
    assert (o.face[0] >= 0).any() and set(np.unique(o.face[0])) >= {0, 1, 6, 7, 8, 10, 11}     # the small ones draw too
    for name in ("switch_strips_h", "switch_strips_v"):
        assert [f for v, f in oracle(name).large if v == 0] == [1]        # 64 x 1 small, 65 x 1 large
        assert (oracle(name).face[0] == 0).sum() == 64 and (oracle(name).face[0] == 1).sum() == 65
    for w in (255, 256, 257, 300):
        o = oracle("wide_row_%d" % w)
        assert (0, 0) in o.large and (o.face[0] >= 0).sum() == w and (o.face[0] == 0).sum() > w - 25
    assert len(oracle("all_large").large) == 3 * RC.ALL_LARGE_FACES and 3 * RC.ALL_LARGE_FACES > 3 * 256
    assert 1 < len(oracle("large_few").large) < 256


def test_incidence_ties_go_to_the_lowest_face_id():
    o, r = oracle("incidence"), oracle("incidence_reversed")
    n = len(RC.scene("incidence").faces)
    assert o.face[0, 6, 6] == 0 and r.face[0, 6, 6] == n - 1 - 5          # the fan's centre: six faces meet, the lowest id wins
    assert list(o.face[0, 6, 7:11]) == [0] * 4 and list(r.face[0, 6, 7:11]) == [n - 1 - 5] * 4      # the spoke faces 0 and 5 share
    assert all(o.face[0, 2 + k, 14 + k] == 6 for k in range(9))           # the square's diagonal: faces 6 and 7
    assert all(r.face[0, 2 + k, 14 + k] == n - 1 - 7 for k in range(9))
    assert np.array_equal(o.depth, r.depth) and np.array_equal(o.face >= 0, r.face >= 0)
    assert np.all(o.face[0, 2:11, 14] >= 0) and np.all(o.face[0, 2:11, 22] >= 0) and np.all(o.face[0, 2, 14:23] >= 0) \
        and np.all(o.face[0, 10, 14:23] >= 0)                             # all four outer sides are drawn: no top-left rule


def test_rotations_and_windings_draw_the_same():
    s, o = RC.scene("rotations"), oracle("rotations")
    st = RC.ROTATION_STEP
    first = slice(0, st)
    assert (o.face[0, :, first] == 0).sum() > 20
    for k, order in enumerate(RC.ROTATION_ORDERS):
        blk = slice(k * st, (k + 1) * st)
        assert np.array_equal(o.depth[0, :, blk], o.depth[0, :, first])
        assert np.array_equal(o.face[0, :, blk] >= 0, o.face[0, :, first] >= 0)
        # vertex ids through the rotation: copy k's vertices are 3k + (0, 1, 2), whatever the order of its face
        hit = o.vid[0, :, first] >= 0
        assert np.array_equal(o.vid[0, :, blk][hit] - 3 * k, o.vid[0, :, first][hit])


def test_rejected_faces_draw_nothing():
    s, o = RC.scene("rejected"), oracle("rejected")
    assert set(np.unique(o.face)) == {-1, *RC.REJECTED_GOOD}
    for vi in range(len(s.views)):
        alone = RX.render_exact(*s.exact[vi], s.faces[list(RC.REJECTED_GOOD)], s.H, s.W, s.znear)
        assert np.array_equal(alone.depth, o.depth[vi]) and np.array_equal(alone.face, o.face[vi])


def test_depth_and_border_rules():
    o = oracle("depth")
    assert not (o.face == 0).any() and (o.face[0] == 1).sum() == 21      # at znear: dropped; one step above: drawn
    assert o.depth[0, 1, 8] == -1.0
    assert not (o.face == 3).any() and (o.face[0] == 2).sum() > 10       # coplanar: the lower id
    assert not (o.face == 5).any() and (o.face[0] == 4).sum() > 10       # equal float32 depths: the lower id, the farther plane
    assert (o.face[0] == 7).sum() > 5 and (o.face[0] == 6).sum() > 0     # nearer wins where both are
    b = oracle("border")
    assert set(np.unique(b.face[0])) == {-1, 0, 1, 2, 6} and b.large == []
    assert b.face[0, 0, 0] == 0 and b.face[0, 8, 8] == 1 and b.face[0, 6, 11] == 1 and list(b.face[0, 1:5, 11]) == [2] * 4
    assert (b.face[0] == 2).sum() == 4 and b.face[0, 8, 4] == 6
    assert oracle("image_1x1").face.shape == (2, 1, 1) and oracle("image_1x1").face[0, 0, 0] == 1


def test_vertex_id_scene_sits_on_its_ties_and_bounds():
    s, o = RC.scene("vertex_ids"), oracle("vertex_ids")
    assert o.face[0, 5, 6] == 0 and o.vid[0, 5, 6] == 2                   # the centroid: all three equal, corner 2
    assert o.vid[0, 3, 4] == 0 and o.vid[0, 6, 7] == 2                    # the median from corner 0: a1 == a2, at the top beyond the
    assert o.vid[0, 3, 10] == 1 and o.vid[0, 6, 4] == 2                   # centroid -> 2; from corner 1: a0 == a2 at the top -> 2
    assert o.vid[0, 9, 4] == 2 and o.vid[0, 3, 7] == 1                    # from corner 2: a0 == a1 at the top -> 1
    assert o.vid[0, 1, 8] == 1                                            # the midpoint of the edge 0-1: a0 == a1 -> 1
    assert o.grey[0, 5, 6] == 255                                         # z == znear_img: inside, white
    assert (o.face[0] == 1).sum() > 5 and set(o.vid[0][o.face[0] == 1]) <= {3, 4, 5} and set(o.grey[0][o.face[0] == 1]) == {0}
    for f in (2, 3):                                                      # one float32 step outside either bound
        assert (o.face[0] == f).sum() > 5 and set(o.vid[0][o.face[0] == f]) == {-1} and set(o.grey[0][o.face[0] == f]) == {0}
    assert oracle("views_17").vid.shape[0] == 17 and oracle("views_17").depth.shape[0] == 16


# ---- mutations of the restatement: each must be caught by a named scene ------------------------------------------------------------
def _edges(u, v, xs, ys):
    return [R.edge(u[a], v[a], u[b], v[b], xs, ys) for a, b in ((1, 2), (2, 0), (0, 1))]


def bary_strict(u, v, A, xs, ys):
    e = _edges(u, v, xs, ys)
    inside = (e[0] > 0) & (e[1] > 0) & (e[2] > 0) if A > 0 else (e[0] < 0) & (e[1] < 0) & (e[2] < 0)
    return inside, e[0] / A, e[1] / A, e[2] / A


def bary_top_left(u, v, A, xs, ys):
    """A half-open fill rule: a pixel on an edge belongs to the triangle only if the edge is a `top` or a `left` one."""
    e = _edges(u, v, xs, ys)
    sg = 1.0 if A > 0 else -1.0
    inside = True
    for ei, (a, b) in zip(e, ((1, 2), (2, 0), (0, 1))):
        du, dv = sg * (u[b] - u[a]), sg * (v[b] - v[a])
        owns = dv > 0 or (dv == 0 and du < 0)
        inside = inside & ((sg * ei > 0) | ((ei == 0) & owns))
    return inside, e[0] / A, e[1] / A, e[2] / A


def _setup_variant(lower=np.ceil, near=lambda z, znear: z > znear):
    def setup(u, v, z, H, W, znear):
        with np.errstate(all="ignore"):
            if not all(near(z[i], znear) and np.isfinite(u[i]) and np.isfinite(v[i]) for i in range(3)):
                return None
            A = (u[2] - u[0]) * (v[1] - v[0]) - (v[2] - v[0]) * (u[1] - u[0])
            if not np.isfinite(A) or A == 0.0:
                return None
            xl, xh = max(0.0, lower(min(u))), min(float(W - 1), np.floor(max(u)))
            yl, yh = max(0.0, lower(min(v))), min(float(H - 1), np.floor(max(v)))
        if not (xl <= xh) or not (yl <= yh):
            return None
        return A, int(xl), int(xh), int(yl), int(yh)
    return setup


def raster_triangle_affine(u, v, z, H, W, znear):
    st = R.setup(u, v, z, H, W, znear)
    if st is None:
        return None
    A, x0, x1, y0, y1 = st
    ys, xs = np.meshgrid(np.arange(y0, y1 + 1, dtype=np.float64), np.arange(x0, x1 + 1, dtype=np.float64), indexing="ij")
    inside, l0, l1, l2 = R.bary(u, v, A, xs, ys)
    z64 = l0 * z[0] + l1 * z[1] + l2 * z[2]
    return x0, y0, inside & (z64 > 0), z64, z64.astype(np.float32)


def winner_ge(a0, a1, a2):
    return np.where((a0 >= a1) & (a0 >= a2), 0, np.where(a1 >= a2, 1, 2))


# name -> (scenes that must catch it, attributes to patch as (module, name, replacement), arguments of restate)
# The exclusive grey bounds use that d is a float32: d >= the double after znear_img is d > znear_img, and the float32 image
# of that double is still (float)znear_img, so nothing but the comparison changes (likewise at zfar_img).
MUTATIONS = {
    "strict edges": (("incidence", "border"), [(R, "bary", bary_strict)], {}),
    "top-left rule": (("incidence", "switch_boxes"), [(R, "bary", bary_top_left)], {}),
    "floor for the box's lower corner": (("switch_boxes",), [(R, "setup", _setup_variant(lower=np.floor))], {}),
    "z >= znear": (("depth",), [(R, "setup", _setup_variant(near=lambda z, znear: z >= znear))], {}),
    "box test on the unclamped box": (("switch_boxes",), [], dict(unclamped=True)),
    "ties to the higher face id": (("incidence", "depth"), [], dict(key="higher_id")),
    "key on the fp64 depth": (("depth",), [], dict(key="f64")),
    "affine depth": (("large_few", "rotations"), [(R, "raster_triangle", raster_triangle_affine)], {}),
    "vertex-id rule with >=": (("vertex_ids",), [(PN, "winner", winner_ge)], {}),
    "grey range exclusive at znear_img": (("vertex_ids",), [], dict(img=(np.nextafter(2.0, 3.0), 4.0))),
    "grey range exclusive at zfar_img": (("vertex_ids",), [], dict(img=(2.0, np.nextafter(4.0, 3.0)))),
}


def test_local_variant_is_the_restatement():
    for name in ("depth", "incidence", "large_few"):
        s = RC.scene(name)
        assert differences(s, restate(s, key="f32")) == []
        for vi in range(len(s.views)):
            d, f = render_keyed(s, vi, "f32")
            assert np.array_equal(d.view(np.uint32), oracle(name).depth[vi].view(np.uint32)) and np.array_equal(f, oracle(name).face[vi])


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_mutation_is_caught(mutation, monkeypatch):
    scenes, patches, kwargs = MUTATIONS[mutation]
    for mod, attr, repl in patches:
        monkeypatch.setattr(mod, attr, repl)
    for name in scenes:
        diff = differences(RC.scene(name), restate(RC.scene(name), **kwargs))
        print("%s: scene %s %s" % (mutation, name, "catches it -- " + "; ".join(diff) if diff else "does NOT catch it"))
        assert diff, "mutation '%s' passes scene %s" % (mutation, name)


# ---- watertightness on non-dyadic input --------------------------------------------------------------------------------------------
def test_sheet_is_watertight_in_the_restatement():
    verts, faces, K, lws, geom = RC.sheet()
    face = R.render(verts, faces, None, K, lws, RC.SHEET_H, RC.SHEET_W, **geom)[2]
    covered, exempt, bad = RC.watertight_report(face)
    print("sheet: %d contained pixels in 3 views, %d exempt, %d faces seen" % (covered, exempt, len(np.unique(face)) - 1))
    assert covered > 500 and len(np.unique(face)) > 150
    assert exempt == 0                                   # the seed is chosen so: no pixel needs the exemption
    assert bad == [], bad[:5]
