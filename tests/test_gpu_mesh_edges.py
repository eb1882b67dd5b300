"""GPU: marching cubes (dfh_mc_count / dfh_mc_emit / dfh_mc_reorder, csrc/dfh_mesh.hip) against the numpy oracle
(oracle/mc_np.py) at the structural edges of the kernels: z rows of 17 and 34 segments of 256 points (the count pass flushes its
packed counters every 16 segments; segments from the 31st on share one activity bit), segments the compacted emit skips in front
of segments it does not, 2048 / 2049 / 4097 tiles with every tile active (the chunks of the hierarchical scan), ragged count-pass
workgroups, volumes behind a misaligned base pointer (the scalar loads for rows the 16-byte loads would take), lattices that are
one point thick after sub-sampling, the fp32 threshold pair at signed zeros, subnormals and levels no float holds, capacities
below the totals behind guard rows, and dfh_mc_reorder on its own across the second round of its block-sum scan.

Faces, vertices and values are bit-equal to the oracle's, normals agree to 2.5e-7 (check_equal of tests/test_gpu_mesh.py)."""
import functools

import numpy as np
import pytest
import torch

from oracle import mc_np
from dynamicfusion_body_amd import _lib, mesh
from dynamicfusion_body_amd.device import current_stream_ptr, dtype_code
from test_gpu_mesh import check_equal

pytestmark = pytest.mark.gpu

ORDERS = ["lattice", "reference"]
NP = {torch.float32: np.float32, torch.float64: np.float64}


@functools.lru_cache(maxsize=None)
def noise(shape, seed, dtype):
    v = np.random.default_rng(seed).normal(size=shape).astype(NP[dtype])
    v.setflags(write=False)
    return v


_oracle_cache = {}


def oracle(vol, level, step=1, order="reference", key=None):
    """mc_np.marching_cubes; with a key, the lattice-order mesh is computed once and shared by the tests of both orders."""
    if key is None:
        lat = mc_np._marching_cubes_lattice(vol, level, step)
    else:
        k = (key, level, step)
        if k not in _oracle_cache:
            _oracle_cache[k] = mc_np._marching_cubes_lattice(vol, level, step)
        lat = _oracle_cache[k]
    return mc_np.reorder_first_use(*lat) if order == "reference" else lat


def dev(vol, offset=0):
    """numpy volume -> contiguous CUDA tensor; offset > 0: a view `offset` elements into a flat buffer (misaligned base)."""
    t = torch.from_numpy(np.array(vol, order="C"))                            # (a copy: the cached volumes are read-only)
    if offset == 0:
        d = t.cuda().contiguous()
        assert d.data_ptr() % 16 == 0
        return d
    flat = torch.zeros(vol.size + offset, dtype=t.dtype, device="cuda")
    d = flat[offset:].view(vol.shape)
    d.copy_(t)
    assert d.is_contiguous() and d.data_ptr() % 16 != 0
    return d


def run(vol, level, step=1, order="reference", visit_all_tiles=False, offset=0):
    return mesh.marching_cubes(dev(vol, offset), level, step, as_numpy=True, order=order, visit_all_tiles=visit_all_tiles)


def check(got, want):
    """check_equal, empty meshes included."""
    if len(want[0]) == 0:
        assert len(want[1]) == 0
        assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2].shape == (0, 3) and got[3].shape == (0,)
        assert got[0].dtype == np.float32 and got[1].dtype == np.int32
        return
    check_equal(got, want)


def noise_case(shape, seed, dtype, level, order, step=1, both_lists=True):
    vol = noise(shape, seed, dtype)
    want = oracle(vol, level, step, order, key=(shape, seed, dtype))
    for visit_all in ((False, True) if both_lists else (False,)):
        check(run(vol, level, step, order, visit_all), want)
    return want


# ---- long rows -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape,seed,nv,nf", [((3, 2, 4200), 0, 27157, 27223), ((2, 3, 8500), 1, 54523, 54902)])
def test_rows_of_17_and_34_segments(shape, seed, nv, nf, dtype, order):
    """4200 points: the count pass's second flush adds to the row's entry (seg >= 16); 8500 points: a third flush, and segments
    31, 32 and 33 share the activity bit.  (The counts are the oracle's for these seeds in lattice order; in white noise at this
    size a float32 copy crosses the level at the same places.)"""
    want = noise_case(shape, seed, dtype, 0.1, order)
    lat = oracle(noise(shape, seed, dtype), 0.1, 1, "lattice", key=(shape, seed, dtype))
    assert (len(lat[0]), len(lat[1])) == (nv, nf)
    assert want[0][:, 2].max() > shape[2] - 8                              # the last segment emits


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_skipped_segments_and_the_shared_activity_bit(dtype, order):
    """One active row neighbourhood whose surface lies in segments 5, 33 and 34 only: the compacted emit skips segments 0-4 and
    6-30 by their own bits, cannot skip 31 and 32 (they share bit 31 with 33 and 34) and finds nothing there; the blob at
    33*256+255 / 34*256 straddles a segment edge, so a cube of segment 33 reads vertex codes of segment 34."""
    vol = np.ones((3, 3, 8800), dtype=NP[dtype])
    zs = (5 * 256 + 17, 33 * 256 + 40, 33 * 256 + 255, 34 * 256)
    for z in zs:
        vol[1, 1, z] = -1.0
    lat = oracle(vol, 0.0, 1, "lattice", key=("blobs", dtype))
    assert (len(lat[0]), len(lat[1])) == (22, 32)
    assert set(np.unique(lat[0][:, 2].astype(np.int64) // 256)) == {5, 33, 34}
    want = oracle(vol, 0.0, 1, order, key=("blobs", dtype))
    assert len(want[0]) == 22
    for visit_all in (False, True):
        check(run(vol, 0.0, 1, order, visit_all), want)


# ---- tile scan, count-pass workgroups -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", [(64, 32, 3), (3, 683, 4), (17, 241, 3), (47, 45, 5)])
def test_scan_chunks_with_every_tile_active(shape, order):
    """2048 tiles (one full chunk; 64 planes: the XCD-interleaved tile numbering of the count pass), 2049 (a second chunk of one
    tile), 4097 (three chunks), 2115; white noise at level 0 makes every tile emit."""
    vol = noise(shape, 21, torch.float32)
    lat = oracle(vol, 0.0, 1, "lattice", key=(shape, 21, torch.float32))
    rows = np.unique((lat[0][:, 0].astype(np.int64)) * shape[1] + lat[0][:, 1].astype(np.int64))
    assert len(rows) >= shape[0] * shape[1] - shape[0] - shape[1]          # (vertices on x / y edges sit in their owner's row)
    noise_case(shape, 21, torch.float32, 0.0, order)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", [(8, 3, 9), (16, 17, 5), (24, 16, 7)])
def test_count_pass_raggedness(shape, order):
    """Fewer than four rows per plane; 17 rows (a wave with one row, three waves idle); plane counts that are multiples of 8."""
    noise_case(shape, 22, torch.float32, 0.0, order)


# ---- misaligned base ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", [(9, 14, 300), (6, 5, 12)])
def test_misaligned_base_takes_the_scalar_loads(shape, order):
    for dtype, offsets in ((torch.float32, (1, 2, 3)), (torch.float64, (1,))):
        vol = noise(shape, 23, dtype)
        want = oracle(vol, 0.0, 1, order, key=(shape, 23, dtype))
        aligned = run(vol, 0.0, 1, order)
        check(aligned, want)
        for off in offsets:
            got = run(vol, 0.0, 1, order, offset=off)
            for a, b in zip(got, aligned):
                assert np.array_equal(a, b), (dtype, off)


# ---- step sub-sampling -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("step", [2, 3, 5])
def test_step_subsampling_float64(step, order):
    noise_case((13, 11, 17), 24, torch.float64, 0.0, order, step=step)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_lattice_one_point_thick(axis, order):
    """step >= a dimension: no cubes (hx, hy or hz false everywhere), only vertices.  Lattice order: the oracle's 21 vertices and
    no faces; reference order drops vertices no face uses: an empty mesh."""
    vol = np.ascontiguousarray(np.moveaxis(noise((2, 9, 9), 0, torch.float32), 0, axis))
    want = oracle(vol, 0.0, 2, order)
    assert len(want[1]) == 0 and len(want[0]) == (21 if order == "lattice" else 0)
    for visit_all in (False, True):
        check(run(vol, 0.0, 2, order, visit_all), want)


# ---- levels -------------------------------------------------------------------------------------------------------------------
def level_volume():
    rng = np.random.default_rng(25)
    vol = rng.normal(size=(8, 7, 12)).astype(np.float32)
    half = rng.random(vol.shape) < 0.3
    vol[half] = np.round(vol[half] * 2) / 2                                   # half-integers, 0.0 and 0.5 among them
    tiny, big = np.float32(2.0 ** -149), np.finfo(np.float32).max
    specials = [0.0, -0.0, tiny, -tiny, big, -big]
    at = rng.permutation(vol.size)[:8 * len(specials)]
    vol.reshape(-1)[at] = np.tile(np.array(specials, dtype=np.float32), 8)
    assert (vol == 0.5).sum() > 5 and np.signbit(vol[vol == 0]).any() and (vol == tiny).sum() == 8
    return vol


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("level", [-0.0, 1e-46, -1e-46, 2.0 ** -149, 0.5, 3.5e38, -3.5e38, float("inf")],
                         ids=["-0.0", "1e-46", "-1e-46", "2^-149", "0.5", "3.5e38", "-3.5e38", "inf"])
def test_float32_thresholds_from_a_double_level(level, order):
    """lo_f / eq_f of mc_params: signed zero, levels below the smallest float32 subnormal (they round to +-0 but separate the
    subnormals from zero differently than 0 does), a subnormal level, a level many samples equal, levels beyond +-FLT_MAX
    (lo_f = FLT_MAX resp. -inf, eq_f = NaN) and +inf.  Whatever the oracle says, empty meshes included."""
    vol = level_volume()
    with np.errstate(all="ignore"):
        want = oracle(vol, level, 1, order)
    if abs(level) > 1e38:
        assert len(want[0]) == 0
    elif level != 0.5:
        assert len(want[0]) > 300
    check(run(vol, level, 1, order), want)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("level", [0.5, 0.0])
def test_float64_samples_equal_to_the_level(level, order):
    """The equality path in the volume's own type: a float64 volume of half-integers."""
    vol = np.round(np.random.default_rng(26).normal(size=(8, 7, 12)) * 2) / 2
    assert (vol == level).sum() > 50
    key = ("half-integers", level)
    assert len(oracle(vol, level, 1, "reference", key=key)[0]) < len(oracle(vol, level, 1, "lattice", key=key)[0])   # degenerate faces dropped, vertices left unused
    check(run(vol, level, 1, order), oracle(vol, level, 1, order, key=key))


# ---- the C entry points ---------------------------------------------------------------------------------------------------------
def test_capacities_below_the_totals_and_no_values_array():
    """dfh_mc_emit with cap_verts / cap_faces below the totals writes the first `cap` rows of the lattice-order mesh and nothing
    else (guard rows behind full-size buffers keep their sentinel); values = NULL changes nothing in the other arrays."""
    lib = _lib.load()
    shape = (14, 13, 12)
    vol_np = noise(shape, 27, torch.float32)
    vol = dev(vol_np)
    res = _lib.iarr(shape)
    nbytes = lib.dfh_mc_workspace_bytes(res, 1)
    ws = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device="cuda")
    totals = torch.zeros(3, dtype=torch.int64, device="cuda")
    _lib.check(lib.dfh_mc_count(vol.data_ptr(), dtype_code(vol), res, 1, 0.1, ws.data_ptr(), nbytes, totals.data_ptr(),
                                current_stream_ptr()), "dfh_mc_count")
    nv, nf, nactive = (int(x) for x in totals.cpu())
    want = oracle(vol_np, 0.1, 1, "lattice")
    assert (nv, nf) == (len(want[0]), len(want[1])) and 0 < nactive <= shape[0] * shape[1]
    guard, fs, isent = 5, -7.5, -12345

    def emit(cap_v, cap_f, with_values=True, n_active=nactive):
        v = torch.full((nv + guard, 3), fs, dtype=torch.float32, device="cuda")
        n = torch.full((nv + guard, 3), fs, dtype=torch.float32, device="cuda")
        val = torch.full((nv + guard,), fs, dtype=torch.float32, device="cuda")
        f = torch.full((nf + guard, 3), isent, dtype=torch.int32, device="cuda")
        _lib.check(lib.dfh_mc_emit(vol.data_ptr(), dtype_code(vol), res, 1, 0.1, ws.data_ptr(), nbytes,
                                   v.data_ptr() if cap_v else None, n.data_ptr() if cap_v else None,
                                   val.data_ptr() if with_values else None, f.data_ptr() if cap_f else None, cap_v, cap_f, n_active,
                                   current_stream_ptr()), "dfh_mc_emit")
        return v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy(), val.cpu().numpy()

    full = emit(nv, nf)
    check_equal((full[0][:nv], full[1][:nf], full[2][:nv], full[3][:nv]), want)
    for a, sent in zip(full, (fs, isent, fs, fs)):
        assert (a[(nf if a is full[1] else nv):] == sent).all()
    for n_active in (nactive, -1):
        for cap_v in (0, 1, nv - 1, nv):
            for cap_f in (0, 1, nf - 1, nf):
                got = emit(cap_v, cap_f, n_active=n_active)
                for a, ref, cap, sent in zip(got, full, (cap_v, cap_f, cap_v, cap_v), (fs, isent, fs, fs)):
                    assert np.array_equal(a[:cap], ref[:cap]), (cap_v, cap_f)
                    assert (a[cap:] == sent).all(), (cap_v, cap_f)
    nov = emit(nv, nf, with_values=False)
    assert (nov[3] == fs).all()
    for a, ref in zip(nov[:3], full[:3]):
        assert np.array_equal(a, ref)


def _reorder(verts, faces, normals, values):
    """dfh_mc_reorder on its own -> (verts, faces, normals, values) as mc_np.reorder_first_use returns them, and used_out."""
    lib = _lib.load()
    nv, nf = len(verts), len(faces)
    dv, dn, dval = (torch.from_numpy(a).cuda() for a in (verts, normals, values))
    df = torch.from_numpy(faces).cuda()
    ov, on, oval = torch.full_like(dv, -7.5), torch.full_like(dn, -7.5), torch.full_like(dval, -7.5)
    nbytes = lib.dfh_mc_reorder_workspace_bytes(nv, nf)
    ws = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device="cuda")
    used = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    ptr = lambda t: t.data_ptr() if t.numel() else None
    _lib.check(lib.dfh_mc_reorder(ptr(dv), ptr(dn), ptr(dval), ptr(df), nv, nf, ptr(ov), ptr(on), ptr(oval), used.data_ptr(),
                                  ws.data_ptr(), nbytes, current_stream_ptr()), "dfh_mc_reorder")
    nu = int(used.item())
    rest = (ov[nu:], on[nu:], oval[nu:])
    assert all(bool((r == -7.5).all()) for r in rest)                        # nothing behind the kept vertices
    return (ov[:nu].cpu().numpy(), df.cpu().numpy(), on[:nu].cpu().numpy(), oval[:nu].cpu().numpy()), nu


@pytest.mark.parametrize("nv,nf,unused", [(120000, 350000, 20000), (500, 341, 100), (500, 342, 100), (40, 0, 0), (0, 0, 0)],
                         ids=["1050000 slots", "1023 slots", "1026 slots", "no faces", "no vertices"])
def test_reorder_on_its_own(nv, nf, unused):
    """Synthetic faces against mc_np.reorder_first_use: 1 050 000 slots = 1 026 block sums (the second 1 024-entry round of
    mc_scan1_kernel), 1023 and 1026 slots (either side of one 1 024-slot block), no faces, no vertices."""
    rng = np.random.default_rng(28)
    usable = np.sort(rng.permutation(nv)[:nv - unused]) if nv else np.zeros(0, dtype=np.int64)
    faces = usable[rng.integers(0, max(len(usable), 1), size=(nf, 3))].astype(np.int32) if nf else np.zeros((0, 3), np.int32)
    verts, normals = rng.normal(size=(nv, 3)).astype(np.float32), rng.normal(size=(nv, 3)).astype(np.float32)
    values = rng.normal(size=(nv,)).astype(np.float32)
    if nf:
        want = mc_np.reorder_first_use(verts, faces, normals, values)
    else:
        want = (verts[:0], faces, normals[:0], values[:0])
    got, nu = _reorder(verts, faces, normals, values)
    assert nu == len(want[0]) and nu <= nv - unused
    if nf > 1000:
        assert nu > 0.9 * (nv - unused)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
