"""CPU: what the marching-cubes entry points (dfh_mc_count / dfh_mc_emit / dfh_mc_reorder, csrc/dfh_mesh.hip) and the band-voxel
extraction entry points (dfh_surface_count / dfh_surface_emit, csrc/dfh_extract.hip) do with arguments they cannot use.
Validation comes before any HIP call, so no GPU is needed: device pointers are dummy non-null integers that nothing
dereferences.  Every refusal returns DFH_E_BADARG and leaves a message naming the entry point; the workspace queries return 0."""
import pytest

from dynamicfusion_body_amd import _lib, build
from test_abi_badargs import OK, PTR, _refused, on_own_thread

G = (6, 5, 8)
NAN, INF = float("nan"), float("inf")
BIG = 1 << 62                                   # a workspace size that no check finds too small
BAD_GRIDS = [(0, 5, 8), (6, 0, 8), (6, 5, 0), (-1, 5, 8), (6, -2, 8), (6, 5, -3)]


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def mc_count(lib, vol=PTR, dtype=_lib.F32, res=G, step=1, level=0.0, ws=PTR, ws_bytes=BIG, totals=PTR):
    return lib.dfh_mc_count(vol, dtype, None if res is None else _lib.iarr(res), step, level, ws, ws_bytes, totals, None)


def mc_emit(lib, vol=PTR, dtype=_lib.F32, res=G, step=1, level=0.0, ws=PTR, ws_bytes=BIG, verts=PTR, normals=PTR, values=PTR, faces=PTR,
            cap_verts=10, cap_faces=10, n_active=0):
    return lib.dfh_mc_emit(vol, dtype, None if res is None else _lib.iarr(res), step, level, ws, ws_bytes, verts, normals, values, faces,
                           cap_verts, cap_faces, n_active, None)


def mc_reorder(lib, verts_in=PTR, normals_in=PTR, values_in=PTR, faces=PTR, n_verts=7, n_faces=9, verts_out=PTR, normals_out=PTR,
               values_out=PTR, used=PTR, ws=PTR, ws_bytes=BIG):
    return lib.dfh_mc_reorder(verts_in, normals_in, values_in, faces, n_verts, n_faces, verts_out, normals_out, values_out, used, ws,
                              ws_bytes, None)


def surface_count(lib, tsdf=PTR, w=PTR, dtype=_lib.F32, res=G, band=1.5, ws=PTR, ws_bytes=BIG, total=PTR):
    return lib.dfh_surface_count(tsdf, w, dtype, None if res is None else _lib.iarr(res), band, ws, ws_bytes, total, None)


def surface_emit(lib, tsdf=PTR, w=PTR, dtype=_lib.F32, res=G, x0=0, band=1.5, ws=PTR, pos=PTR, nrm=PTR, capacity=0):
    return lib.dfh_surface_emit(tsdf, w, dtype, None if res is None else _lib.iarr(res), x0, band, ws, pos, nrm, capacity, None)


@on_own_thread
def test_mc_count_refusals(lib):
    name = "dfh_mc_count"
    for null in ("vol", "res", "ws", "totals"):
        _refused(lib, name, mc_count(lib, **{null: None}))
    for dtype in (-1, 2, 7):
        _refused(lib, name, mc_count(lib, dtype=dtype))
    for res in BAD_GRIDS:
        _refused(lib, name, mc_count(lib, res=res))
    for step in (0, -1):
        _refused(lib, name, mc_count(lib, step=step))
    _refused(lib, name, mc_count(lib, level=NAN))
    need = lib.dfh_mc_workspace_bytes(_lib.iarr(G), 1)
    for short in (0, need - 1):
        _refused(lib, name, mc_count(lib, ws_bytes=short))
    _refused(lib, name, mc_count(lib, ws_bytes=lib.dfh_mc_workspace_bytes(_lib.iarr(G), 2)))      # sized for a coarser lattice
    _refused(lib, name, mc_count(lib, res=(1 << 30, 64, 2)))                                      # 2^32 count-pass workgroups


@on_own_thread
def test_mc_emit_refusals_and_nothing_to_do(lib):
    name = "dfh_mc_emit"
    for null in ("vol", "res", "ws"):
        _refused(lib, name, mc_emit(lib, **{null: None}))
    for dtype in (-1, 2):
        _refused(lib, name, mc_emit(lib, dtype=dtype))
    for res in BAD_GRIDS:
        _refused(lib, name, mc_emit(lib, res=res))
    for step in (0, -4):
        _refused(lib, name, mc_emit(lib, step=step))
    need = lib.dfh_mc_workspace_bytes(_lib.iarr(G), 1)
    for short in (0, need - 1):
        _refused(lib, name, mc_emit(lib, ws_bytes=short))
    _refused(lib, name, mc_emit(lib, cap_verts=-1))
    _refused(lib, name, mc_emit(lib, cap_faces=-1))
    _refused(lib, name, mc_emit(lib, cap_verts=1 << 29))                   # vertex ids share a word with a 3-bit mask
    _refused(lib, name, mc_emit(lib, cap_verts=1 << 40))
    for null in ("verts", "normals"):
        _refused(lib, name, mc_emit(lib, **{null: None}))
    _refused(lib, name, mc_emit(lib, faces=None))
    _refused(lib, name, mc_emit(lib, n_active=G[0] * G[1] + 1))            # more active tiles than tiles
    _refused(lib, name, mc_emit(lib, res=(13, 11, 17), step=3, n_active=5 * 4 + 1))
    _refused(lib, name, mc_emit(lib, res=(1 << 20, 1 << 14, 2), n_active=-1))   # every tile: 2^32 workgroups
    # no active tile: nothing to do, with exactly-sized workspace, the largest capacity, without values, with null outputs and no capacity
    assert mc_emit(lib, ws_bytes=need, cap_verts=(1 << 29) - 1, values=None) == OK
    assert mc_emit(lib, verts=None, normals=None, values=None, faces=None, cap_verts=0, cap_faces=0) == OK
    assert mc_emit(lib, verts=None, normals=None, cap_verts=0) == OK and mc_emit(lib, faces=None, cap_faces=0) == OK


@on_own_thread
def test_mc_reorder_refusals(lib):
    name = "dfh_mc_reorder"
    for sizes in ({"n_verts": -1}, {"n_faces": -1}, {"n_verts": 1 << 31}, {"n_faces": ((1 << 32) - 1 + 2) // 3}, {"n_faces": 1 << 40}):
        _refused(lib, name, mc_reorder(lib, **sizes))
    for null in ("used", "ws"):
        _refused(lib, name, mc_reorder(lib, **{null: None}))
    need = lib.dfh_mc_reorder_workspace_bytes(7, 9)
    for short in (0, need - 1):
        _refused(lib, name, mc_reorder(lib, ws_bytes=short))
    _refused(lib, name, mc_reorder(lib, n_verts=8, ws_bytes=lib.dfh_mc_reorder_workspace_bytes(3, 9)))
    for null in ("verts_in", "normals_in", "verts_out", "normals_out"):
        _refused(lib, name, mc_reorder(lib, **{null: None}))
    _refused(lib, name, mc_reorder(lib, faces=None))


@on_own_thread
def test_surface_count_refusals(lib):
    name = "dfh_surface_count"
    for null in ("tsdf", "w", "res", "ws", "total"):
        _refused(lib, name, surface_count(lib, **{null: None}))
    for dtype in (-1, 2):
        _refused(lib, name, surface_count(lib, dtype=dtype))
    for res in BAD_GRIDS:
        _refused(lib, name, surface_count(lib, res=res))
    for band in (0.0, -0.0, -1.5, NAN, -INF):
        _refused(lib, name, surface_count(lib, band=band))
    need = lib.dfh_surface_workspace_bytes(_lib.iarr(G))
    for short in (0, need - 1):
        _refused(lib, name, surface_count(lib, ws_bytes=short))
    _refused(lib, name, surface_count(lib, res=(1 << 30, 1 << 30, 1)))     # 2^50 blocks


@on_own_thread
def test_surface_emit_refusals_and_nothing_to_do(lib):
    name = "dfh_surface_emit"
    for null in ("tsdf", "w", "res", "ws"):
        _refused(lib, name, surface_emit(lib, **{null: None}))
    for dtype in (-1, 2):
        _refused(lib, name, surface_emit(lib, dtype=dtype))
    for res in BAD_GRIDS:
        _refused(lib, name, surface_emit(lib, res=res))
    for band in (0.0, -1.5, NAN):
        _refused(lib, name, surface_emit(lib, band=band))
    _refused(lib, name, surface_emit(lib, capacity=-1))
    _refused(lib, name, surface_emit(lib, capacity=5, pos=None))
    _refused(lib, name, surface_emit(lib, capacity=5, nrm=None))
    assert surface_emit(lib, capacity=0, pos=None, nrm=None) == OK         # nothing to write: no output arrays needed
    assert surface_emit(lib, capacity=0, band=INF) == OK


@on_own_thread
def test_workspace_queries(lib):
    """0 for sizes they cannot use (and no message: they are queries), growing with the grid otherwise."""
    mc = lambda res, step=1: lib.dfh_mc_workspace_bytes(None if res is None else _lib.iarr(res), step)
    sf = lambda res: lib.dfh_surface_workspace_bytes(None if res is None else _lib.iarr(res))
    assert mc(None) == 0 and sf(None) == 0
    for res in BAD_GRIDS:
        assert mc(res) == 0 and sf(res) == 0
    assert mc(G, 0) == 0 and mc(G, -1) == 0
    for n_verts, n_faces in ((-1, 0), (0, -1), (-5, -5)):
        assert lib.dfh_mc_reorder_workspace_bytes(n_verts, n_faces) == 0
    assert lib.dfh_mc_reorder_workspace_bytes(0, 0) > 0
    grids = [(1, 1, 1), (2, 2, 2), (6, 5, 8), (6, 5, 9), (6, 6, 9), (7, 6, 9), (64, 32, 3), (3, 683, 4), (64, 64, 64), (128, 128, 256), (129, 128, 256)]
    for a, b in zip(grids, grids[1:]):
        assert 0 < mc(a) <= mc(b) and 0 < sf(a) <= sf(b), (a, b)
    assert mc((64, 64, 64)) > mc((6, 5, 8)) and sf((129, 128, 256)) > sf((128, 128, 256))
    assert mc((13, 11, 17), 1) > mc((13, 11, 17), 2) >= mc((13, 11, 17), 3) >= mc((13, 11, 17), 17) > 0
    sizes = [(0, 0), (1, 0), (1, 1), (100, 341), (100, 342), (101, 342), (120000, 350000)]
    for a, b in zip(sizes, sizes[1:]):
        assert lib.dfh_mc_reorder_workspace_bytes(*a) <= lib.dfh_mc_reorder_workspace_bytes(*b), (a, b)
    assert lib.dfh_mc_reorder_workspace_bytes(120000, 350000) >= 4 * (2 * 120000 + 1026 + 1)               # first use, new id, 1026 block sums
