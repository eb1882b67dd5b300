"""GPU: K24, mesh simplification by vertex clustering with quadrics (csrc/dfh_mesh_simplify.hip) against tests/simplify_np.py, bit
for bit on every output -- positions, faces, face_idx, vert_map, attributes, cluster and fall-back counts -- at the shapes where
it can go wrong (tests/simplify_cases.py), then what the device refuses and the three simplify_cell hooks."""
import json
import os

import numpy as np
import pytest
import torch

import simplify_np as SN
from simplify_cases import CASES, REG_CASES, cube_side
from dynamicfusion_body_amd import Fusion, FusionDM, mesh

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simplify_recovery.json")
MODES = ("quadric", "mean")


def attributes(v):
    """Two per-vertex attributes of a case: (V, 3) float32 and (V,) float64."""
    v = np.asarray(v, dtype=np.float64)
    return (np.cos(v * 1.3) + 0.25).astype(np.float32), v[:, 0] * 0.37 - v[:, 2] if len(v) else np.zeros(0)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_equal(got, want, what):
    *mesh_out, info = got
    v, f, attrs = mesh_out[0], mesh_out[1], mesh_out[2:]
    assert all(t.is_cuda for t in mesh_out) and info["vert_map"].is_cuda and info["face_idx"].is_cuda, what
    assert (info["n_clusters"], info["n_fallback"]) == (want["n_clusters"], want["n_fallback"]), what
    assert f.dtype == torch.int32 and tuple(f.shape) == want["faces"].shape and np.array_equal(f.cpu().numpy(), want["faces"]), what
    assert info["face_idx"].dtype == torch.int64 and np.array_equal(info["face_idx"].cpu().numpy(), want["face_idx"]), what
    assert info["vert_map"].dtype == torch.int64 and np.array_equal(info["vert_map"].cpu().numpy(), want["vert_map"]), what
    gv = v.cpu().numpy()
    assert gv.dtype == want["verts"].dtype and gv.shape == want["verts"].shape and np.array_equal(raw(gv), raw(want["verts"])), what
    assert len(attrs) == len(want["attrs"]), what
    for a, w in zip(attrs, want["attrs"]):
        ga = a.cpu().numpy()
        assert ga.dtype == w.dtype and ga.shape == w.shape and np.array_equal(raw(ga), raw(w)), what


def runs(name):
    return [(mode, reg) for mode in MODES for reg in ((1e-3, 0.0) if name in REG_CASES and mode == "quadric" else (1e-3,))]


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_output_equals_the_restatement(name):
    v, f, cell, origin = CASES[name]
    attrs = attributes(v)
    for mode, reg in runs(name):
        for drop in (True, False):
            want = SN.simplify(v, f, attrs, cell=cell, origin=origin, mode=mode, reg=reg, drop_unreferenced=drop)
            got = mesh.simplify(v, f, *attrs, cell=cell, origin=origin, mode=mode, reg=reg, drop_unreferenced=drop)
            assert_equal(got, want, (name, mode, reg, drop))


@pytest.mark.parametrize("name", ["cube", "lattice_cell2", "fan_hub_last", "crowded_cell", "thin_sheet", "strip_1025", "isolated_unreferenced"])
def test_float32_vertices_and_attributes_are_widened_exactly_and_come_back_float32(name):
    v, f, cell, origin = CASES[name]
    v32 = v.astype(np.float32)
    a32 = attributes(v)[0]
    for mode in MODES:
        want = SN.simplify(v32, f, (a32,), cell=cell, origin=origin, mode=mode)
        got = mesh.simplify(torch.from_numpy(v32).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(a32).cuda(), cell=cell, origin=origin, mode=mode)
        assert got[0].dtype == torch.float32 and got[2].dtype == torch.float32
        assert_equal(got, want, (name, mode))


def test_int64_faces_and_tensors_are_accepted():
    v, f, cell, origin = CASES["lattice_80x40_cell1.5"]
    got = mesh.simplify(torch.from_numpy(v), torch.from_numpy(f.astype(np.int64)).cuda(), cell=cell)
    assert_equal(got, SN.simplify(v, f, cell=cell), "int64 faces")


@pytest.mark.parametrize("name", ["cube_permuted", "fan_hub_last", "crowded_cell", "lattice_80x40_cell1.5", "thin_sheet"])
def test_the_same_call_twice_gives_the_same_bits(name):
    v, f, cell, origin = CASES[name]
    a = mesh.simplify(v, f, v, cell=cell, origin=origin)
    b = mesh.simplify(v, f, v, cell=cell, origin=origin)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
    assert torch.equal(a[3]["vert_map"], b[3]["vert_map"]) and torch.equal(a[3]["face_idx"], b[3]["face_idx"])
    assert (a[3]["n_clusters"], a[3]["n_fallback"]) == (b[3]["n_clusters"], b[3]["n_fallback"])


def test_reg_0_on_the_plane_falls_back_to_the_mean_through_the_pivot_test():
    v, f, cell, origin = CASES["plane"]
    q = mesh.simplify(v, f, cell=cell, origin=origin, reg=0.0, drop_unreferenced=False)
    m = mesh.simplify(v, f, cell=cell, origin=origin, mode="mean", drop_unreferenced=False)
    assert q[2]["n_fallback"] == q[2]["n_clusters"] > 0 and m[2]["n_fallback"] == 0
    assert torch.equal(q[0].view(torch.int64), m[0].view(torch.int64))
    assert mesh.simplify(v, f, cell=cell, origin=origin, reg=1e-3)[2]["n_fallback"] == 0


def test_the_thin_sheet_keeps_the_lower_of_two_opposite_faces():
    v, f, cell, origin = CASES["thin_sheet"]
    nv, nf, info = mesh.simplify(v, f, cell=cell, origin=origin)
    assert 0 < len(nf) and int(info["face_idx"].max()) < len(f) // 2      # every survivor is from the first sheet


def test_a_vertex_permutation_keeps_the_membership_and_numbers_by_lowest_index():
    from simplify_cases import cube, permuted
    v, f = cube()
    pv, pf, perm = permuted(v, f)
    a = mesh.simplify(v, f, cell=3.0, drop_unreferenced=False)[2]
    b = mesh.simplify(pv, pf, cell=3.0, drop_unreferenced=False)[2]
    va, vb = a["vert_map"].cpu().numpy(), b["vert_map"].cpu().numpy()
    assert a["n_clusters"] == b["n_clusters"] == 152
    group = lambda vc, ident: sorted(sorted(ident[np.nonzero(vc == c)[0]].tolist()) for c in range(vc.max() + 1))
    assert group(va, np.arange(len(v))) == group(vb, perm)
    firsts = [np.nonzero(vb == c)[0].min() for c in range(b["n_clusters"])]
    assert firsts == sorted(firsts)


def test_the_quadric_representative_recovers_the_cube_corners():
    v, f, cell, origin = CASES["cube"]
    q = SN.cube_measures(mesh.simplify(v, f, cell=cell, mode="quadric")[0].cpu().numpy(), *cube_side())
    m = SN.cube_measures(mesh.simplify(v, f, cell=cell, mode="mean")[0].cpu().numpy(), *cube_side())
    print("corner distance: quadric %.6f, mean %.6f" % (q["corner_distance_max"], m["corner_distance_max"]))
    assert q["corner_distance_max"] < 0.1 * m["corner_distance_max"]
    want = json.load(open(GOLDEN))["cube"]
    assert q == want["quadric"] and m == want["mean"]         # the same bits as the restatement, so the same figures


REFUSED = {
    "a NaN coordinate": lambda v, f: (np.where(np.arange(v.size).reshape(v.shape) == 3 * 700 + 1, np.nan, v), f, 3.0),
    "an infinite coordinate": lambda v, f: (np.where(np.arange(v.size).reshape(v.shape) == 5, np.inf, v), f, 3.0),
    "a cell coordinate of 2^21": lambda v, f: (np.concatenate([v, [[0.25, 0.25, 0.25 + 1e-3 * ((1 << 21) + 5)]]]), f, 1e-3),
    "a face index of V": lambda v, f: (v, np.concatenate([f[:1500], [[0, 1, len(v)]], f[1500:]]).astype(np.int32), 3.0),
    "a negative face index": lambda v, f: (v, np.concatenate([f, [[0, -1, 2]]]).astype(np.int32), 3.0),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_the_device_refuses_without_a_fault(what):
    v, f, _, _ = CASES["cube"]
    bv, bf, cell = REFUSED[what](v, f)
    with pytest.raises(ValueError, match="dfh_mesh_simplify_keys"):
        mesh.simplify(bv, bf, cell=cell)
    with pytest.raises(ValueError):
        SN.simplify(bv, bf, cell=cell)
    assert_equal(mesh.simplify(v, f, cell=3.0), SN.simplify(v, f, cell=3.0), "after a refusal")


def test_a_cell_coordinate_just_below_2_21_is_accepted():
    v, f, _, _ = CASES["triangle_three_cells"]
    far = np.concatenate([v, [[0.1, 0.1, 0.1 + 0.5 * ((1 << 21) - 1)]]])
    assert_equal(mesh.simplify(far, f, cell=0.5, origin=(0.0, 0.0, 0.0)), SN.simplify(far, f, cell=0.5, origin=(0.0, 0.0, 0.0)), "2^21 - 1")


# ---- the hooks, on an analytic sphere at 32^3 ---------------------------------------------------------------------------------
CELL = 2.0


def sphere_volume():
    g = np.stack(np.meshgrid(*[np.arange(32.0)] * 3, indexing="ij"), axis=-1)
    return np.clip(np.linalg.norm(g - np.array([15.3, 15.6, 15.4]), axis=-1) - 9.2, -3.0, 3.0).astype(np.float32)


def make(cls, vol):
    if cls == "Fusion":
        return Fusion(vol.copy(), 3.0, subsample_rate=2.0, knn=4, marching_cubes_step_size=1, write_warpfield=False)
    fu = FusionDM(3.0, np.array([[100.0, 0, 16], [0, 100.0, 16], [0, 0, 1]]), tsdf_res=32, marching_cubes_step_size=1, write_warpfield=False)
    fu._ensure_volumes()
    fu._T.copy_(torch.from_numpy(vol))
    return fu


@pytest.mark.parametrize("cls", ["Fusion", "FusionDM"])
def test_write_canonical_mesh_writes_the_simplified_mesh_and_leaves_the_stored_one(cls, tmp_path):
    fu = make(cls, sphere_volume())
    fu.marching_cubes()
    v0, f0 = fu._vertices.copy(), fu._faces.copy()
    assert fu.simplify_cell is None
    fu.write_canonical_mesh(str(tmp_path), "plain.obj")      # before the attribute is touched
    fu.simplify_cell = CELL
    fu.write_canonical_mesh(str(tmp_path), "coarse.obj")
    assert np.array_equal(fu._vertices, v0) and np.array_equal(fu._faces, f0)
    fu.simplify_cell = None
    fu.write_canonical_mesh(str(tmp_path), "again.obj")
    assert np.array_equal(fu._vertices, v0) and np.array_equal(fu._faces, f0)
    assert open(tmp_path / "plain.obj", "rb").read() == open(tmp_path / "again.obj", "rb").read()
    pv, pf, pn = mesh.read_obj(str(tmp_path / "plain.obj"))
    cv, cf, cn = mesh.read_obj(str(tmp_path / "coarse.obj"))
    assert 0 < len(cf) < len(pf) and 0 < len(cv) < len(pv) and len(cn) == len(cv)
    length = np.linalg.norm(np.asarray(cn, dtype=np.float64), axis=1)
    assert (((np.abs(length - 1.0) < 1e-5) | (length == 0.0))).all()     # unit or zero, to the six decimals of the file
    if cls == "Fusion":                                      # an index-space file: distances in voxels
        T = torch.from_numpy(sphere_volume()).cuda()
        mv, mf, _, _ = mesh.marching_cubes(T, None, 1)
        d = mesh.surface_distance(np.asarray(cv, dtype=np.float64), mv.cpu().numpy(), mf.cpu().numpy())
        print("simplified vertices to the unsimplified surface: mean %.6f max %.6f voxel (%d -> %d faces)" % (float(d.mean()), float(d.max()), len(pf), len(cf)))
        # a new vertex lies in a cell that holds an original vertex: at most the cell's diagonal away (+ the file's %f rounding)
        assert float(d.max()) <= np.sqrt(3.0) * CELL + 1e-6
        want = json.load(open(GOLDEN))["hooks"]
        assert [len(pf), len(cf)] == want["faces_before_after"]
        assert float(d.mean()) == pytest.approx(want["surface_distance_mean"], rel=1e-3)


def test_colored_mesh_simplifies_before_it_samples_the_colours():
    from dynamicfusion_body_amd import kernels
    from dynamicfusion_body_amd.pipeline import SlabFrame
    sf = SlabFrame.__new__(SlabFrame)
    sf.ws = 1
    sf.T = torch.from_numpy(sphere_volume()).cuda()
    sf.C = kernels.color_volume((32, 32, 32))
    sf.C[..., 0] = 4.0 * torch.arange(32.0, device="cuda")[:, None, None]
    sf.C[..., 1], sf.C[..., 2], sf.C[..., 3] = 20.0, 30.0, 1.0
    v0, f0, n0, rgb0, ok0 = sf.colored_mesh()
    wv, wf, wn, _ = mesh.marching_cubes(sf.T, 0.0, 1)
    assert torch.equal(v0, wv) and torch.equal(f0, wf) and torch.equal(n0, wn)
    v1, f1, n1, rgb1, ok1 = sf.colored_mesh(simplify_cell=CELL)
    sv, sf_, sn, _ = mesh.simplify_with_normals(wv, wf, wn, CELL)
    assert torch.equal(v1, sv) and torch.equal(f1, sf_) and torch.equal(n1, sn) and 0 < len(f1) < len(f0)
    assert rgb1.shape == v1.shape and n1.shape == v1.shape and ok1.shape == (len(v1),) and int(f1.max()) == len(v1) - 1
    rgb, ok = kernels.sample_colors(sf.C, v1.double())       # the colour volume at the new vertices
    assert torch.equal(ok1, ok) and torch.equal(rgb1[ok1], rgb[ok]) and bool(ok1.any())
    length = torch.linalg.vector_norm(n1.double(), dim=1)
    assert bool((((length - 1.0).abs() < 1e-6) | (length == 0)).all())
