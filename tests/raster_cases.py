"""Rasterizer scenes that are exact in fp64, for tests/test_raster_exact.py (CPU) and tests/test_gpu_raster_edges.py (GPU).

A scene is written down in the screen space of its first view: vertices at (u, v, z) with u, v on a quarter-pixel grid and z a
power of two (a few scenes use other depths of few bits and say so).  Every view has a power-of-two focal length, an integer or
half-integer principal point, a rotation that is a 90-degree turn about the optical axis and a dyadic translation, and the
voxel -> world map is scale = 1/64, half = 32 with a dyadic centre (some scenes use the identity map).  The voxel-space
vertices x = (u - cx) z / f etc. are computed here in Fractions and must be doubles; so are the projections into every view,
which the CPU test compares with render_np.project bit for bit: the device's projection of these scenes has no rounding error,
and the exact oracle (tests/raster_exact.py) sees the same triangles as the kernel.  Everything is generated from integers.
"""
import functools
from fractions import Fraction as Fr

import numpy as np

GEOM = dict(scale=1.0 / 64, half=32.0, center=(0.25, -0.5, 0.125))
IDENT = dict(scale=1.0, half=0.0, center=(0.0, 0.0, 0.0))
TURNS = ((1, 0, 0, 1), (0, -1, 1, 0), (-1, 0, 0, -1), (0, 1, -1, 0))          # (r00, r01, r10, r11) of a turn about the axis
INT32_MAX = 2 ** 31 - 1
Q = Fr(1, 4)


class View:
    def __init__(self, cx, cy, turn=0, t=(0, 0, 0), f=32):
        self.f, self.cx, self.cy, self.turn, self.t = Fr(f), Fr(cx), Fr(cy), turn % 4, tuple(Fr(c) for c in t)

    def K(self):
        return np.array([[float(self.f), 0.0, float(self.cx)], [0.0, float(self.f), float(self.cy)], [0.0, 0.0, 1.0]])

    def lw(self):
        a, b, c, d = TURNS[self.turn]
        return np.array([[a, b, 0, float(self.t[0])], [c, d, 0, float(self.t[1])], [0, 0, 1, float(self.t[2])]], dtype=np.float64)

    def to_camera(self, w):
        a, b, c, d = TURNS[self.turn]
        return (a * w[0] + b * w[1] + self.t[0], c * w[0] + d * w[1] + self.t[1], w[2] + self.t[2])

    def to_world(self, cam):
        a, b, c, d = TURNS[self.turn]
        x, y = cam[0] - self.t[0], cam[1] - self.t[1]
        return (a * x + c * y, b * x + d * y, cam[2] - self.t[2])             # R^T


class Scene:
    """name, H, W, views, znear, geom (scale / half / center), img = (znear_img, zfar_img); after finish(): verts (n, 3) float64,
    faces (m, 3) int32, exact[view] = (u, v, z) lists of Fractions (None for a vertex that is not finite), normals / cpos /
    cnrm (n, 3) float64 per-vertex attributes."""

    def __init__(self, name, H, W, views, znear=0.5, geom=GEOM, img=(2.0, 4.0)):
        self.name, self.H, self.W, self.views, self.znear, self.geom, self.img = name, H, W, list(views), znear, geom, img
        self._uvz, self._raw, self._faces = [], {}, []

    # ---- building ---------------------------------------------------------------------------------------------------------------
    def vert(self, u, v, z=2):
        self._uvz.append((Fr(u), Fr(v), Fr(z)))
        return len(self._uvz) - 1

    def raw_vert(self, xyz):
        """A vertex given by voxel-space coordinates that are not finite."""
        self._raw[len(self._uvz)] = tuple(xyz)
        self._uvz.append(None)
        return len(self._uvz) - 1

    def face(self, i, j, k):
        self._faces.append((i, j, k))
        return len(self._faces) - 1

    def tri(self, p0, p1, p2, z=2, order=(0, 1, 2)):
        """Three new vertices p = (u, v) or (u, v, z) and the face through them in `order`; z one depth or three."""
        zs = z if isinstance(z, tuple) else (z, z, z)
        ids = [self.vert(*(p if len(p) == 3 else (p[0], p[1], zz))) for p, zz in zip((p0, p1, p2), zs)]
        return self.face(*(ids[o] for o in order))

    def box(self, x0, y0, w, h, z=2, corner=0):
        """A right triangle whose bounding box is exactly w x h pixels with its lower corner at (x0, y0); z one depth or three."""
        x1, y1 = x0 + w - 1, y0 + h - 1
        c = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
        return self.tri(*(c[(corner + j) % 4] for j in (0, 1, 3)), z=z)

    def finish(self):
        b = self.views[0]
        sc, hf, ce = Fr(self.geom["scale"]), Fr(self.geom["half"]), [Fr(c) for c in self.geom["center"]]
        n = len(self._uvz)
        self.verts = np.zeros((n, 3))
        for i, p in enumerate(self._uvz):
            if p is None:
                self.verts[i] = self._raw[i]
                continue
            u, v, z = p
            w = b.to_world(((u - b.cx) * z / b.f, (v - b.cy) * z / b.f, z))
            for c in range(3):
                q = (w[c] - ce[c]) / sc + hf
                self.verts[i, c] = float(q)
                assert Fr(self.verts[i, c]) == q, "%s: vertex %d is not a double" % (self.name, i)
        self.faces = np.array(self._faces, dtype=np.int64).reshape(-1, 3).astype(np.int32)
        self.exact = []
        for vw in self.views:
            U, V, Z = [], [], []
            for i, p in enumerate(self._uvz):
                if p is None:
                    U.append(None), V.append(None), Z.append(None)
                    continue
                w = [sc * (Fr(self.verts[i, c]) - hf) + ce[c] for c in range(3)]
                cam = vw.to_camera(w)
                U.append(vw.f * cam[0] / cam[2] + vw.cx), V.append(vw.f * cam[1] / cam[2] + vw.cy), Z.append(cam[2])
            self.exact.append((U, V, Z))
        i = np.arange(n, dtype=np.int64)
        self.normals = np.stack([(i * 7) % 9 - 4, (i * 5) % 7 - 3, 8 + (i * 3) % 5], axis=1) / 8.0
        self.cpos = np.stack([(i * 37 + 11) % 101 - 50, (i * 53 + 7) % 97 - 48, (i * 29 + 3) % 89 - 44], axis=1) / 8.0
        self.cnrm = np.stack([(i * 11 + 2) % 13 - 6, 9 + (i * 3) % 4, (i * 17 + 5) % 11 - 5], axis=1) / 16.0
        return self

    # ---- what the calls take ----------------------------------------------------------------------------------------------------
    def Ks(self, views=None):
        return np.stack([v.K() for v in (self.views if views is None else views)])

    def lws(self, views=None):
        return np.stack([v.lw() for v in (self.views if views is None else views)])


T0 = (Fr(1, 4), Fr(-1, 8), Fr(1, 2))                   # a dyadic translation: 32 * t / z stays on the quarter grid up to z = 16


def _two_views(cx, cy):
    """A turned first view and a second one that is another turn, another principal point and a sideways step."""
    return [View(cx, cy, turn=1, t=T0), View(cx - 1, cy + Fr(1, 2), turn=0, t=(Fr(-1, 8), Fr(1, 4), Fr(1, 2)))]


# ---- small / large switch ---------------------------------------------------------------------------------------------------------
def switch_boxes():
    s = Scene("switch_boxes", 40, 48, _two_views(24, Fr(39, 2)))
    s.box(1, 10, 8, 8)                                  # 64: small
    s.box(11, 10, 4, 16, z=4)                           # 64: small
    s.box(17, 10, 5, 13, z=(2, 4, 2))                   # 65: large
    s.box(24, 10, 9, 8, z=(4, 2, 1), corner=2)          # 72: large
    for ox, oy in ((2, 28), (36, 28)):                  # one triangle with u in [ox, ox + 8], v in [oy, oy + 7]: 9 x 8, large
        s.tri((ox, oy), (ox + 8, oy), (ox, oy + 7))
    s.tri((12 + Q, 28), (20 + Q, 28), (12 + Q, 35))    # the same a quarter pixel to the right: columns 13..20, 8 x 8, small
    s.tri((24, 28 + Q), (32, 28 + Q), (24, 35 + Q))    # and a quarter pixel down: rows 29..35, 9 x 7, small
    s.tri((1, -3), (8, -3), (1, 7))                     # 8 x 11 before the clamp, rows 0..7 after it: 64, small
    s.tri((12, -2), (19, -2), (12, 8))                  # one pixel further down: rows 0..8, 72, large
    s.tri((-3, 1), (7, 1), (-3, 8), z=4)                # 11 x 8 before the clamp, columns 0..7 after it: small
    s.tri((40, 1), (49, 1), (40, 8), z=4)               # 10 x 8 before, columns 40..47 after: small
    s.tri((39, 19), (49, 19), (39, 26), z=4)            # 11 x 8 before, columns 39..47 after: large
    return s.finish()


def switch_strips(vertical):
    """Boxes of 64 x 1 and 65 x 1 pixels (1 x 64 and 1 x 65 when vertical): slivers half a pixel thick with the apex on a pixel
    centre."""
    H, W = (70, 5) if vertical else (5, 70)
    s = Scene("switch_strips_v" if vertical else "switch_strips_h", H, W, [View(2, 2, turn=3, t=T0), View(3, 2, turn=3, t=T0)])
    for row, length, z in ((1, 64, 2), (3, 65, (2, 2, 4))):
        p = [(2, row - Q), (2, row + Q), (2 + length - 1, row)]
        if vertical:
            p = [(b, a) for a, b in p]
        s.tri(*p, z=z)
    return s.finish()


# ---- large-path shapes ------------------------------------------------------------------------------------------------------------
def wide(width, vertical=False):
    """One box of `width` x 1 pixels in an image of 1 x 300 (300 x 1 when vertical), tilted in depth, with two small occluders;
    a second view one and three pixels aside clips it."""
    H, W = (300, 1) if vertical else (1, 300)
    name = "wide_col_%d" % width if vertical else "wide_row_%d" % width
    a = (300 - width) // 2
    views = [View(0, 150, turn=2), View(0, 151, turn=2), View(0, 147, turn=2)] if vertical else \
            [View(150, 0, turn=2), View(151, 0, turn=2), View(147, 0, turn=2)]
    s = Scene(name, H, W, views)
    tris = [([(a, -2 * Q), (a, 2 * Q), (a + width - 1, 0)], (2, 2, 4)),
            ([(40, -Q), (47, -Q), (40, 3 * Q)], (1, 1, 1)),
            ([(250, -3 * Q), (262, 0), (250, 3 * Q)], (1, 2, 1))]
    for p, z in tris:
        if vertical:
            p = [(y, x) for x, y in p]
        s.tri(*p, z=z)
    return s.finish()


def large_few():
    """Six large triangles in two views: fewer than 256 pairs, so one workgroup pulls the whole list.  A 37 x 29 box (1 073
    pixels: more than four lane-steps, ending inside one; 37 does not divide 256), tilted depths over {1, 2, 4}, occluders."""
    s = Scene("large_few", 40, 48, [View(Fr(47, 2), 20, turn=2, t=T0), View(Fr(47, 2), 19, turn=0, t=(Fr(1, 8), 0, Fr(1, 2)))])
    s.box(3, 4, 37, 29, z=(4, 2, 4))
    s.box(5, 2, 37, 29, z=(1, 4, 2), corner=2)
    s.tri((2, 3), (45 + Q, 20 + 2 * Q), (8 + 3 * Q, 38 + Q), z=4, order=(0, 2, 1))
    s.tri((30, 1, 2), (46, 12, 4), (20 + Q, 30, 1))
    s.box(10, 10, 13, 7, z=1)                           # occluders in front of part of them
    s.box(25, 22, 11, 9, z=(1, 2, 1), corner=1)
    s.box(20, 16, 5, 5, z=1, corner=3)                  # a small one
    return s.finish()


ALL_LARGE_FACES = 260                                   # not a multiple of 256: a workgroup of the small kernel spans two views


def all_large():
    """Every triangle is large in every view: 3 views x 260 faces = 780 pairs, a raster grid of ceil(780 / 256) = 4 workgroups
    that take about 195 listed pairs each.  The views are turns about the centre of a square image, so boxes keep their size."""
    c = Fr(25, 2)
    s = Scene("all_large", 26, 26, [View(c, c, turn=0, t=(0, 0, Fr(1, 2))), View(c, c, turn=1, t=(0, 0, Fr(1, 2))),
                                    View(c, c, turn=2, t=(0, 0, Fr(1, 2)))])
    shapes = ((9, 8), (5, 13), (13, 5), (8, 9), (11, 6), (7, 10))
    for i in range(ALL_LARGE_FACES):
        w, h = shapes[i % 6]
        x0, y0 = (i * 7 + 3) % (26 - w + 1), (i * 11 + 5) % (26 - h + 1)
        z = tuple(2 ** ((i * m + k) % 3) for m, k in ((1, 0), (3, 1), (5, 2)))
        s.box(x0, y0, w, h, z=z, corner=i % 4)
    return s.finish()


# ---- pixel-centre incidence -------------------------------------------------------------------------------------------------------
def incidence(reverse=False):
    s = Scene("incidence_reversed" if reverse else "incidence", 20, 24, _two_views(12, Fr(19, 2)))
    # a fan of six around a vertex on the pixel centre (6, 6), all at one depth; the spokes to (10, 6) and (2, 6) run through
    # pixel centres
    c = s.vert(6, 6)
    ring = [s.vert(6 + dx, 6 + dy) for dx, dy in ((4, 0), (2, Fr(7, 2)), (-2, Fr(7, 2)), (-4, 0), (-2, Fr(-7, 2)), (2, Fr(-7, 2)))]
    fan = [(c, ring[k], ring[(k + 1) % 6]) for k in range(6)]
    # a square cut along its 45-degree diagonal, which runs through pixel centres; its sides are horizontal and vertical outer
    # edges through pixel centres
    q = [s.vert(14, 2), s.vert(22, 2), s.vert(22, 10), s.vert(14, 10)]
    quad = [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    # two triangles either side of a horizontal edge through pixel centres, and two either side of a vertical one
    h = [s.vert(2, 14), s.vert(10, 14), s.vert(6, 18), s.vert(6, 11)]
    v = [s.vert(17, 12), s.vert(17, 19), s.vert(13, 15), s.vert(22, 16)]
    pairs = [(h[0], h[1], h[2]), (h[1], h[0], h[3]), (v[0], v[1], v[2]), (v[0], v[1], v[3])]
    faces = fan + quad + pairs
    for f in (faces[::-1] if reverse else faces):
        s.face(*f)
    return s.finish()


ROTATION_ORDERS = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1))
ROTATION_STEP = 10


def rotations():
    """One tilted triangle four times, ten pixels apart: the three rotations of its vertex order and the other winding."""
    s = Scene("rotations", 12, 40, [View(20, 6, turn=3, t=T0)])
    for k, order in enumerate(ROTATION_ORDERS):
        o = ROTATION_STEP * k
        s.tri((1 + o, 1, 1), (8 + Q + o, 2 + 2 * Q, 2), (3 + o, 9 + 3 * Q, 4), order=order)
    return s.finish()


# ---- image border -----------------------------------------------------------------------------------------------------------------
def border():
    """Identity voxel -> world map and a principal point of (0, 0), so that a voxel coordinate of -0.0 is a screen coordinate."""
    s = Scene("border", 9, 12, [View(0, 0), View(1, 2)], geom=IDENT)
    s.tri((0, 0), (3, 0), (0, 3))                       # u = 0 and v = 0 (and a voxel coordinate set to -0.0 below)
    s.tri((8, 5), (11, 6), (8, 8))                      # u = W - 1 and v = H - 1
    s.tri((11, 1), (14, 2), (11, 4), z=4)               # smallest u = W - 1: a box of one column
    s.tri((-3, 2), (-Q, 3), (-2, 5))                    # largest u = -0.25: nothing
    s.tri((5 + Q, 1), (5 + 3 * Q, 1), (5 + 2 * Q, 6))   # between two pixel columns: an empty box
    s.tri((1, 6 + Q), (4, 6 + 2 * Q), (2, 6 + 3 * Q))   # between two pixel rows
    s.tri((4, 8), (7, 8), (5, 12), z=4)                 # smallest v = H - 1: a box of one row
    s.finish()
    assert s.verts[0, 0] == 0.0 and s.verts[2, 0] == 0.0 and s.verts[0, 1] == 0.0
    s.verts[0, 0] = s.verts[0, 1] = s.verts[2, 0] = -0.0
    return s


def image_1x1():
    s = Scene("image_1x1", 1, 1, _two_views(0, 0))
    s.tri((-9, -7), (11, -5), (-2, 14), z=4)            # around the pixel
    s.tri((0, 0), (3, 1), (1, 3), z=(2, 1, 1))          # a vertex on the pixel centre
    s.tri((Q, Q), (3, 1), (1, 3), z=1)                  # misses it
    s.tri((-1, 0), (1, 0), (0, -2), z=8)                # an edge through it, behind
    return s.finish()


# ---- depth ------------------------------------------------------------------------------------------------------------------------
def depth():
    """znear = 1.  Depths that are not powers of two have few bits and sit at u, v that keep the products exact (the CPU test
    checks the projection of every scene)."""
    s = Scene("depth", 12, 20, [View(0, 0, turn=1), View(0, 0, turn=1, f=64)], znear=1.0, geom=IDENT)
    above = 1 + Fr(1, 2 ** 52)                          # one float64 step above znear
    s.tri((1, 1, 1), (6, 1, 2), (1, 6, 2))              # a vertex at exactly znear: dropped (the rule needs z > znear)
    s.tri((8, 1, above), (13, 1, 2), (8, 6, 2))         # its twin one step above: drawn
    s.tri((1, 7), (7, 7), (1, 11))                      # two coplanar faces at equal depth: the lower id wins
    s.tri((1, 7), (7, 7), (1, 11))
    far = 2 * (1 + Fr(1, 2 ** 30))                      # rounds to float32 2.0, well inside the cell
    s.tri((10, 7), (18, 7), (10, 11), z=far)            # the farther plane has the lower id: equal float32 depths, it wins
    s.tri((10, 7), (18, 7), (10, 11), z=2)
    s.tri((14, 1), (19, 1), (14, 5), z=4)               # plainly behind
    s.tri((15, 2), (19, 2), (15, 5), z=2)               # plainly in front of it
    return s.finish()


# ---- rejected faces among good ones -----------------------------------------------------------------------------------------------
REJECTED_GOOD = (0, 1, 2)                               # the faces of `rejected` that draw


def rejected():
    s = Scene("rejected", 16, 24, _two_views(12, Fr(15, 2)))
    s.tri((1, 1), (12, 2), (3, 13), z=(2, 4, 2))
    s.tri((10, 5), (22, 3), (20, 14), z=(1, 2, 4))
    s.tri((4, 9), (15, 8), (9, 15), z=4)
    bad = [s.raw_vert((np.nan, 40.0, 100.0)), s.raw_vert((30.0, np.inf, 100.0)), s.raw_vert((30.0, 40.0, -np.inf))]
    a, m, b = s.vert(1, 1, 2), s.vert(7, 7, 2), s.vert(13, 13, 2)      # collinear on the grid
    n = len(s._uvz)
    s.face(0, 1, -1), s.face(n, 3, 4), s.face(6, INT32_MAX, 7)          # vertex indices outside [0, n_verts)
    s.face(0, 1, bad[0]), s.face(bad[1], 4, 5), s.face(6, bad[2], 8)    # NaN, +inf and -inf coordinates
    s.face(0, 0, 1), s.face(3, 4, 4)                                    # a repeated vertex
    s.face(a, m, b)
    return s.finish()


# ---- vertex ids -------------------------------------------------------------------------------------------------------------------
def _shift_views(n, cx, cy):
    """n views: integer shifts of the principal point combined with the four turns, a step aside in every third."""
    return [View(cx + (i % 5) - 2 + (Fr(1, 2) if i % 2 else 0), cy + (i % 3) - 1, turn=i % 4,
                 t=(Fr(i % 3, 8), Fr(-(i % 2), 4), Fr(1, 2))) for i in range(n)]


def vertex_ids():
    """The image range is [2, 4].  A flat triangle at z = 2 = znear_img whose centroid (6, 5) and medians lie on pixel centres;
    planes at zfar_img and one float32 step outside either bound (depths of few bits, not powers of two)."""
    s = Scene("vertex_ids", 16, 20, [View(10, 8, turn=1, t=(0, 0, Fr(1, 2))), View(9, Fr(15, 2), turn=3, t=(0, 0, Fr(1, 2)))],
              img=(2.0, 4.0))
    s.tri((2, 1), (14, 1), (2, 13), z=2)
    s.tri((15, 1), (19, 1), (15, 5), z=4)               # exactly zfar_img: grey 0, a vertex id
    s.tri((15, 6), (19, 6), (15, 10), z=2 * (1 - Fr(1, 2 ** 24)))     # the float32 below 2: outside
    s.tri((15, 11), (19, 11), (15, 15), z=4 * (1 + Fr(1, 2 ** 23)))   # the float32 above 4: outside
    s.tri((4, 9, 2), (13, 10, 4), (6, 15, 2))           # tilted, partly behind the first
    return s.finish()


def views(n):
    """n views of a handful of tilted triangles, one of them large (n = 16: one call; n = 17: two batches of the vertex-id
    wrapper)."""
    s = Scene("views_%d" % n, 16, 20, _shift_views(n, 10, 8), img=(1.0, 3.0))
    s.tri((2, 1, 2), (17, 3, 4), (5, 14, 1))
    s.tri((1, 8, 1), (9, 6, 2), (7, 15, 2))
    s.tri((10, 2), (18, 2), (18, 10), z=2)
    s.tri((10, 2), (18, 10), (10, 10), z=2)
    s.tri((12, 9, 4), (19, 12, 1), (11, 15, 2), order=(0, 2, 1))
    return s.finish()


BUILDERS = {
    "switch_boxes": switch_boxes,
    "switch_strips_h": functools.partial(switch_strips, False),
    "switch_strips_v": functools.partial(switch_strips, True),
    "wide_row_255": functools.partial(wide, 255),
    "wide_row_256": functools.partial(wide, 256),
    "wide_row_257": functools.partial(wide, 257),
    "wide_row_300": functools.partial(wide, 300),
    "wide_col_300": functools.partial(wide, 300, True),
    "large_few": large_few,
    "all_large": all_large,
    "incidence": incidence,
    "incidence_reversed": functools.partial(incidence, True),
    "rotations": rotations,
    "border": border,
    "image_1x1": image_1x1,
    "depth": depth,
    "rejected": rejected,
    "vertex_ids": vertex_ids,
    "views_16": functools.partial(views, 16),
    "views_17": functools.partial(views, 17),
}
NAMES = tuple(BUILDERS)
RENDER_MAX_VIEWS = 16                                   # views per raster call; views_17 is rendered as its first 16 there


@functools.lru_cache(maxsize=None)
def scene(name):
    s = BUILDERS[name]()
    assert s.name == name
    return s


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The exact oracle's results of a scene (raster_exact.SceneOracle): computed once, shared by every test, never changed."""
    import raster_exact
    return raster_exact.render_scene(scene(name))


# ---- the non-dyadic sheet of the watertightness check ---------------------------------------------------------------------------
SHEET_H, SHEET_W, SHEET_SEED = 30, 41, 5


@functools.lru_cache(maxsize=None)
def sheet():
    """A jittered 14 x 14 grid sheet with alternating diagonals; row 6 is moved to within 1e-13 of row 5 (a row of slivers).
    Returns (verts, faces, K, lws, geom): a skewed general K and three turned views."""
    rng = np.random.default_rng(SHEET_SEED)
    n = 14
    gy, gx = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    P = np.stack([gx * 0.11 - 0.7, gy * 0.1 - 0.66, 2.0 + 0.05 * np.sin(gx) + 0.03 * gy], axis=-1)
    P += rng.uniform(-0.02, 0.02, P.shape)
    P[6] = P[5] + np.array([0.0, 1e-13, 0.0])
    verts = (P.reshape(-1, 3) - np.array(GEOM["center"])) / GEOM["scale"] + GEOM["half"]
    faces = []
    for j in range(n - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i
            faces += [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
    K = np.array([[27.3, 0.71, 20.4], [0.0, 24.9, 14.2], [0.0, 0.0, 1.0]])
    lws = []
    for ang, t in ((0.0, (0.0, 0.0, 0.0)), (0.31, (0.1, -0.05, 0.2)), (-0.47, (-0.15, 0.1, 0.4))):
        c, s_ = np.cos(ang), np.sin(ang)
        Ry = np.array([[c, 0, s_], [0, 1, 0], [-s_, 0, c]])
        cz, sz = np.cos(0.4 * ang + 0.1), np.sin(0.4 * ang + 0.1)
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        R = Rz @ Ry
        pivot = np.array([0.0, 0.0, 2.0])
        lws.append(np.concatenate([R, (pivot - R @ pivot + np.array(t))[:, None]], axis=1))
    return verts, np.array(faces, dtype=np.int32), K, np.array(lws), GEOM


@functools.lru_cache(maxsize=None)
def sheet_coverage():
    """Per view of the sheet: raster_exact.coverage_exact_on_doubles of render_np.project's doubles."""
    import raster_exact
    import render_np
    verts, faces, K, lws, geom = sheet()
    out = []
    for lw in lws:
        U, V, _ = render_np.project(verts, K, lw, **geom)
        out.append(raster_exact.coverage_exact_on_doubles(U, V, faces, SHEET_H, SHEET_W))
    return out


def watertight_report(face_maps):
    """A (3, H, W) face map of the sheet against the exact coverage: (pixels some closed triangle contains, exempt pixels,
    violations as strings).  Every contained pixel must be covered, every other pixel empty, and the winning face one of the
    faces that contain the pixel.  A pixel is exempt only if one of its exact edge values is below the rounding bound of the
    edge expression."""
    covered = exempt = 0
    bad = []
    for vi, cov in enumerate(sheet_coverage()):
        for y in range(SHEET_H):
            for x in range(SHEET_W):
                entries = cov.get((y, x), [])
                inside = {f for f, ins, _ in entries if ins}
                covered += bool(inside)
                got = int(face_maps[vi, y, x])
                if any(abs(e) < b for _, _, es in entries for e, b in es):
                    exempt += 1
                elif inside and got < 0:
                    bad.append("view %d pixel (%d, %d): a hole, faces %s contain it" % (vi, x, y, sorted(inside)))
                elif not inside and got >= 0:
                    bad.append("view %d pixel (%d, %d): face %d drawn, no triangle contains it" % (vi, x, y, got))
                elif inside and got not in inside:
                    bad.append("view %d pixel (%d, %d): face %d does not contain it" % (vi, x, y, got))
    return covered, exempt, bad
