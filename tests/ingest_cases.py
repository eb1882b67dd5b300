"""Fixtures of the RGB-D ingest tests: cases whose decisions sit exactly on, and on each side of, a boundary of the header's
text (tests/test_ingest.py checks on the restatement that they do; tests/test_gpu_ingest.py compares the device with the
restatement on them), and seeded random frames for the size sweeps.

The boundary cases use power-of-two intrinsics and depths, so that us, vs, u and v are exact: out pinhole fx = fy = 64,
cx = cy = 0, depth_scale = 2^-10 and raw values whose z is a power of two.  Expected values come from Python's Fraction
arithmetic and round() (half to even on exact rationals), not from numpy."""
from fractions import Fraction

import numpy as np

import ingest_np as N

OUT_K = (64.0, 64.0, 0.0, 0.0)
SCALE = 2.0 ** -10
EPS = 2.0 ** -40


def _case(raw, img, views, check, **kw):
    kw.setdefault("depth_scale", SCALE)
    return {"args": (np.asarray(raw, dtype=np.uint16), None if img is None else np.asarray(img, dtype=np.uint8), views, OUT_K),
            "kw": kw, "check": check}


def _coded_raw(V, H, W):
    """raw[v][sj][si] = 1024 + 32*sj + si + 1000*v: the value names the source pixel."""
    sj, si = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([(1024 + 32 * sj + si + 1000 * v).astype(np.uint16) for v in range(V)])


def source_ties():
    """us = 1.5 i + c, vs = 1.5 j + c per view, c = -2, 0 and each +-2^-40: x.5 ties (2.5 -> 2, 5.5 -> 6), -0.5 (-> -0: inside)
    and Wd - 0.5 = 8.5 at Wd = 9 (-> 8: inside), Hd - 0.5 = 7.5 at Hd = 8 (-> 8: outside), with a case on each side of each."""
    H, W = 8, 9
    cs = [Fraction(-2), Fraction(0), Fraction(-2) + Fraction(1, 2 ** 40), Fraction(-2) - Fraction(1, 2 ** 40),
          Fraction(1, 2 ** 40), -Fraction(1, 2 ** 40)]
    raw = _coded_raw(len(cs), H, W)
    views = [N.view((96.0, 96.0, float(c), float(c))) for c in cs]

    def check(out):
        depth = out[0]
        n_tie = n_edge = 0
        for v, c in enumerate(cs):
            for j in range(H):
                for i in range(W):
                    us, vs = Fraction(3, 2) * i + c, Fraction(3, 2) * j + c
                    si, sj = round(us), round(vs)
                    inside = 0 <= si <= W - 1 and 0 <= sj <= H - 1
                    want = np.float32(-(float(raw[v, sj, si]) * SCALE)) if inside else np.float32(0)
                    assert depth[v, j, i] == want, (v, j, i, us, vs)
                    n_tie += us.denominator == 2 or vs.denominator == 2
                    n_edge += us in (Fraction(-1, 2), Fraction(17, 2)) or vs in (Fraction(-1, 2), Fraction(15, 2))
        assert n_tie >= 40 and n_edge >= 20, (n_tie, n_edge)
        assert depth[0, 1, 1] == np.float32(-(float(raw[0, 0, 0]) * SCALE))            # (-0.5, -0.5) reads pixel (0, 0)
        assert depth[0, 2, 7] == np.float32(-(float(raw[0, 1, 8]) * SCALE))            # us = 8.5 reads column 8
        assert depth[1, 5, 1] == 0 and depth[3, 1, 1] == 0 and depth[2, 1, 1] != 0     # vs = 7.5 -> 8; -0.5 - eps -> -1; -0.5 + eps -> 0
    return _case(raw, None, views, check)


def _flat_colour(H, W):
    col = np.arange(W)[None, :, None] + 7 * np.arange(3)[None, None, :] + 0 * np.arange(H)[:, None, None]
    return col.astype(np.uint8)


def colour_edges():
    """T_dc = identity, z = 1 exactly, fc = (64, 64, c, 0): u = i + c, v = j.  c = 0: u = 0 is inside, u = Wc - 1 is not; c = -2^-40
    pushes column 0 out and column Wc - 1 in; c = +2^-40 does neither."""
    H, W = 6, 8
    cs = [0.0, -EPS, EPS]
    raw = np.full((len(cs), H, W), 1024, dtype=np.uint16)
    img = np.stack([_flat_colour(H, W)] * len(cs))
    views = [N.view(OUT_K, fc=(64.0, 64.0, c, 0.0)) for c in cs]

    def check(out):
        has = out[1][..., 3] == 255
        for v, c in enumerate(cs):
            want = np.zeros((H, W), dtype=bool)
            for i in range(W):
                u = Fraction(i) + Fraction(c)
                want[:H - 1, i] = 0 <= u < W - 1                     # (v = j: the last row is outside whatever the column)
            assert np.array_equal(has[v], want), (v, has[v])
        assert has[0, 0, 0] and not has[0, 0, W - 1] and not has[1, 0, 0] and has[1, 0, W - 1] and has[2, 0, 0] and not has[2, 0, W - 1]
        assert np.array_equal((out[2] != 0), has)
    return _case(raw, img, views, check, occl_tol=0.0, sample=0)


def z_range():
    """z_min = 1, z_max = 2 with raw 1023 | 1024 | 2048 | 2049 | 0 | 65535: exactly on a bound is valid, one device unit beyond is not."""
    raw = np.array([[[1023, 1024, 2048, 2049], [0, 65535, 1024, 2048]]], dtype=np.uint16)

    def check(out):
        want = np.array([[0, -1.0, -2.0, 0], [0, 0, -1.0, -2.0]], dtype=np.float32)
        assert np.array_equal(out[0][0], want)
    return _case(raw, None, [N.view(OUT_K)], check, z_min=1.0, z_max=2.0)


def raw_extremes():
    """No upper bound: raw = 65535 is a measurement (z = 65535 / 1024 exactly), raw = 0 never is, whatever z_min."""
    raw = np.array([[[0, 65535, 1], [65535, 0, 1]]], dtype=np.uint16)

    def check(out):
        want = np.array([[0, -65535.0 / 1024, -1.0 / 1024], [-65535.0 / 1024, 0, -1.0 / 1024]], dtype=np.float32)
        assert np.array_equal(out[0][0], want) and not np.signbit(out[0][0][0, 0])
    return _case(raw, None, [N.view(OUT_K)], check, z_min=0.0, z_max=0.0)


def _occlusion(tol, occluded):
    """Column 3 at z = 1, the rest at z = 2, T_dc = a shift of 1/32 along x: a pixel lands at u = i + 2 / z, so column 4 (z = 2,
    u = 5) lies behind column 3 (z = 1, u = 5).  Its own key is 2.0 and the buffer holds 1.0: occluded iff 1.0 + occl_tol < 2.0."""
    H, W = 5, 10
    raw = np.full((1, H, W), 2048, dtype=np.uint16)
    raw[0, :, 3] = 1024
    img = _flat_colour(H, W)[None]
    T = np.hstack([np.eye(3), np.array([[1.0 / 32], [0.0], [0.0]])])

    def check(out):
        depth, color, cdepth, zbuf = out
        has = color[0][..., 3] == 255
        assert has[0, 3] and color[0][0, 3, 0] == 5                 # the front pixel takes colour column 5
        assert has[0, 4] == (not occluded)
        assert zbuf[0][0, 5] == np.float32(1.0).view(np.uint32)
        if not occluded:
            assert color[0][0, 4, 0] == 5 and cdepth[0][0, 4] == depth[0][0, 4] == -2.0
        else:
            assert cdepth[0][0, 4] == 0 and depth[0][0, 4] == -2.0
    return _case(raw, img, [N.view(OUT_K, fc=OUT_K, T=T)], check, occl_tol=tol, sample=0, max_splat=8)


def bilinear_ties():
    """fc cx = cy = 0.5: fu = fv = 0.5 at every pixel, the image steps by 1 per column and 2 per row: every channel of every
    pixel is k + 1.5 exactly on .5 (10.5 -> 10, 11.5 -> 12)."""
    H, W = 6, 9
    raw = np.full((1, H, W), 1024, dtype=np.uint16)
    img = (_flat_colour(H, W).astype(np.int64) + 2 * np.arange(H)[:, None, None]).astype(np.uint8)[None]

    def check(out):
        color = out[1][0]
        n = 0
        for j in range(H - 1):
            for i in range(W - 1):
                assert color[j, i, 3] == 255
                for ch in range(3):
                    t = [Fraction(int(img[0, j + a, i + b, ch])) for a in (0, 1) for b in (0, 1)]
                    c = sum(t) / 4
                    assert c.denominator == 2
                    assert color[j, i, ch] == round(c), (j, i, ch, c)
                    n += 1
        assert n >= 80
        assert (color[H - 1:] == 0).all() and (color[:, W - 1:] == 0).all()           # u = Wc - 0.5 in the last column: outside
    return _case(raw, img, [N.view(OUT_K, fc=(64.0, 64.0, 0.5, 0.5))], check, occl_tol=0.0, sample=1)


BOUNDARY_CASES = {
    "source_ties": source_ties,
    "colour_edges": colour_edges,
    "z_range": z_range,
    "raw_extremes": raw_extremes,
    "occl_tol_equal": lambda: _occlusion(1.0, False),
    "occl_tol_below": lambda: _occlusion(1.0 - EPS, True),
    "bilinear_ties": bilinear_ties,
}


# ---- seeded frames for the size sweeps and the geometry edges ---------------------------------------------------------------------
def random_frame(seed, V, depth_size, color_size=None, C=3, distortion=False, ratio=None, T=None, invalid=0.1):
    """V views of a random scene: raw depth around 1-3 m with steps and holes, random colour images, per-view intrinsics a few
    per cent apart.  ratio: colour focal length / depth focal length (default: the images' width ratio).
    -> (raw (V, Hd, Wd) uint16, img (V, Hc, Wc, C) uint8 or None, views, out_k)"""
    rng = np.random.default_rng(seed)
    Hd, Wd = depth_size
    f = 0.9 * max(Hd, Wd, 8)
    out_k = (f, f, (Wd - 1) / 2.0, (Hd - 1) / 2.0)
    jj, ii = np.meshgrid(np.arange(Hd), np.arange(Wd), indexing="ij")
    raws, imgs, views = [], [], []
    for v in range(V):
        base = 1500 + 400 * np.sin(ii / 7.0 + v) + 300 * np.cos(jj / 5.0)
        base = np.where((ii // 6 + jj // 5 + v) % 4 == 0, base + 900, base)           # steps: foreground against background
        raw = np.rint(base + rng.integers(-20, 21, size=base.shape)).astype(np.uint16)
        raw[rng.random(base.shape) < invalid] = 0
        raws.append(raw)
        fd = (f * (1 + 0.03 * rng.standard_normal()), f * (1 + 0.03 * rng.standard_normal()),
              out_k[2] + rng.uniform(-1, 1), out_k[3] + rng.uniform(-1, 1))
        kd = (0.1, -0.05, 1e-3, -1e-3, 0.01) if distortion else (0,) * 5
        fc, kc, Tv = (1.0, 1.0, 0.0, 0.0), (0,) * 5, None
        if color_size is not None:
            Hc, Wc = color_size
            r = Wc / float(Wd) if ratio is None else ratio
            fc = (f * r * (1 + 0.02 * rng.standard_normal()), f * r * (1 + 0.02 * rng.standard_normal()),
                  (Wc - 1) / 2.0 + rng.uniform(-1, 1), (Hc - 1) / 2.0 + rng.uniform(-1, 1))
            kc = (-0.08, 0.03, -5e-4, 7e-4, -0.005) if distortion else (0,) * 5
            a = 0.02 * rng.standard_normal()
            Tv = np.array([[np.cos(a), 0.0, np.sin(a), 0.05], [0.0, 1.0, 0.0, -0.01], [-np.sin(a), 0.0, np.cos(a), 0.005]]) if T is None else T
            imgs.append(rng.integers(0, 256, size=(Hc, Wc, C)).astype(np.uint8))
        views.append(N.view(fd, kd, fc, kc, Tv))
    return np.stack(raws), np.stack(imgs) if imgs else None, views, out_k
