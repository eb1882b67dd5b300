"""CPU: the rasterizer's C ABI (dfh_render_*) is declared, exported and bound, and its numpy restatement (tests/render_np.py,
the yardstick of tests/test_gpu_render.py) gets cases with known answers right.  No compute entry point is called."""
import ctypes

import numpy as np
import pytest

import render_np as RN
from dynamicfusion_body_amd import _lib, build

RENDER_SYMBOLS = ("dfh_render_workspace_bytes", "dfh_render_raster", "dfh_render_resolve")


@pytest.fixture(scope="module")
def lib_path():
    return build.build_library()


def test_render_symbols_declared_exported_bound_at_abi8(lib_path):
    """The rasterizer's entry points (added with ABI 5) are declared, exported and bound in the library of ABI 8 (7 passed the
    GN problem and live frame as structs, 8 the slab, volume, views and nodes of K1-K3)."""
    declared = _lib.declared_symbols()
    lib = ctypes.CDLL(lib_path)
    for name in RENDER_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib._SIGNATURES, name
    assert _lib.ABI_VERSION == 8 and _lib.load().dfh_version() == 8


def test_render_workspace_size_query(lib_path):
    """The size query needs no device: keys (8 B per pixel and view) plus the large-triangle list; bad sizes give 0."""
    lib = _lib.load()
    n = lib.dfh_render_workspace_bytes(3, 240, 320, 1000)
    assert n >= 3 * 240 * 320 * 8 + 3 * 1000 * 4
    assert lib.dfh_render_workspace_bytes(0, 240, 320, 10) == 0
    assert lib.dfh_render_workspace_bytes(17, 240, 320, 10) == 0
    assert lib.dfh_render_workspace_bytes(1, 0, 320, 10) == 0


# camera: f = 64, principal point at the origin, identity pose; world points at z = 2 land on pixel u = 32 x
K64 = np.array([[64.0, 0.0, 0.0], [0.0, 64.0, 0.0], [0.0, 0.0, 1.0]])
LW_ID = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)


def test_fronto_parallel_quad_is_exact_and_has_no_holes():
    """Two triangles sharing the diagonal of a square at z = 2 (corners on pixel centres u in {8, 40}, v in {4, 36}): every
    pixel of the closed square carries exactly -2, the diagonal included (inclusive rule), nothing outside; where both
    triangles cover a pixel the lower face id wins."""
    Z = 2.0
    corners = np.array([[8, 4], [40, 4], [40, 36], [8, 36]], dtype=np.float64)
    verts = np.concatenate([corners * Z / 64.0, np.full((4, 1), Z)], axis=1)
    for faces in (np.array([[0, 1, 2], [0, 2, 3]]), np.array([[0, 2, 1], [0, 3, 2]])):      # both windings
        depth, _, face = RN.render(verts, faces, None, K64, LW_ID, 48, 48)
        inside = np.zeros((48, 48), dtype=bool)
        inside[4:37, 8:41] = True
        assert np.all(depth[0][inside] == -2.0)
        assert np.all(depth[0][~inside] == 0.0) and np.all(face[0][~inside] == -1)
        ys, xs = np.nonzero(inside)
        on_diag = (xs - 8) == (ys - 4)
        assert np.all(face[0][ys[on_diag], xs[on_diag]] == 0)
        assert set(np.unique(face[0][inside])) == {0, 1}


def test_tilted_plane_matches_ray_plane_depth():
    """One large triangle on the plane n . X = d seen through a general K and pose: the fp64 perspective-correct depth of
    every covered pixel equals the ray-plane intersection to 1e-12 relative."""
    K = np.array([[300.5, 0.25, 160.3], [0.0, 301.25, 119.7], [0.0, 0.0, 1.0]])
    a = np.radians(10.0)
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    lw = np.concatenate([R, np.array([[0.05], [-0.02], [0.3]])], axis=1)
    verts = np.array([[-0.6, -0.5, 2.2], [0.7, -0.4, 1.7], [0.1, 0.6, 2.6]])
    U, V, Zc = RN.project(verts, K, lw, 1.0, 0.0, 0.0)
    r = RN.raster_triangle(U, V, Zc, 240, 320, 1e-3)
    assert r is not None
    x0, y0, ok, z64, _ = r
    assert ok.sum() > 1000
    cam = verts @ R.T + lw[:, 3]
    n = np.cross(cam[1] - cam[0], cam[2] - cam[0])
    d = n @ cam[0]
    ys, xs = np.nonzero(ok)
    rays = np.stack([xs + x0, ys + y0, np.ones_like(xs)], axis=-1).astype(np.float64) @ np.linalg.inv(K).T    # ray z = 1
    z_ref = d / (rays @ n)
    assert np.abs(z64[ok] - z_ref).max() <= 1e-12 * np.abs(z_ref).max()


def test_degenerate_and_near_plane_triangles_draw_nothing():
    Z = 2.0
    p = lambda u, v, z=Z: [u * z / 64.0, v * z / 64.0, z]
    verts = np.array([p(8, 8), p(30, 8), p(8, 30),          # 0-2: a proper triangle (drawn)
                      p(10, 10), p(20, 20), p(30, 30),      # 3-5: collinear
                      p(12, 5), p(12, 5), p(25, 20),        # 6-8: repeated vertex
                      [0.1, 0.1, 1e-4], p(30, 8), p(8, 30), # 9: a vertex closer than znear
                      [0.1, 0.1, -1.0], p(30, 8), p(8, 30), # 12: a vertex behind the camera
                      [0.0, 0.0, 0.0], p(30, 8), p(8, 30)]) # 15: a vertex at the camera centre (z = 0)
    for tri in ([3, 4, 5], [6, 7, 8], [9, 10, 11], [12, 13, 14], [15, 16, 17], [0, 1, 99]):
        depth, _, face = RN.render(verts, np.array([tri]), None, K64, LW_ID, 48, 48)
        assert np.all(depth == 0) and np.all(face == -1), tri
    depth, _, face = RN.render(verts, np.array([[0, 1, 2]]), None, K64, LW_ID, 48, 48)
    assert (face == 0).sum() > 200 and np.all(depth[face == 0] == -2.0)
