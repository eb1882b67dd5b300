"""GPU: K25, mesh smoothing by Taubin's lambda|mu filter over a fixed Laplacian and area-weighted vertex normals
(csrc/dfh_mesh_smooth.hip) against tests/smooth_np.py, bit for bit on every output -- positions, attributes of width 1 and 4, the
boundary flags, the normals -- at the shapes where it can go wrong (tests/smooth_cases.py), then what the device refuses, the
recovery figures, the stored marching-cubes mesh and the three smooth_iters hooks."""
import json
import os

import numpy as np
import pytest
import torch

import smooth_np as SN
from smooth_cases import CASES, CENTRE, RADIUS, noisy_icosphere
from dynamicfusion_body_amd import Fusion, FusionDM, mesh

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WEIGHTS, BOUNDARY, ITERS, MUS = ("uniform", "cotangent"), ("fixed", "free"), (0, 1, 3), (None, 0.0)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(t, want):
    got = t.cpu().numpy()
    return t.is_cuda and got.dtype == want.dtype and got.shape == want.shape and np.array_equal(raw(got), raw(want))


def attributes(v, dtype=np.float64):
    """Two per-vertex attributes of a case: (V,) and (V, 4)."""
    v = np.asarray(v, dtype=np.float64)
    one = v[:, 0] * 0.37 - v[:, 2] if len(v) else np.zeros(0)
    four = np.concatenate([np.cos(v * 1.3) + 0.25, np.sin(v[:, :1] + v[:, 1:2])], axis=1)
    return one.astype(dtype), four.astype(dtype)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_output_equals_the_restatement(name):
    v, f = CASES[name]
    a1, a4 = attributes(v)
    for weights in WEIGHTS:
        for boundary in BOUNDARY:
            want = SN.Laplacian(v, f, weights, boundary)
            got = mesh.MeshLaplacian(v, f, weights, boundary)
            assert got.boundary.dtype == torch.bool and same(got.boundary, want.boundary), (name, weights, boundary)
            for sign in (1.0, -1.0):
                assert same(got.vertex_normals(sign=sign), want.vertex_normals(sign=sign)), (name, weights, sign)
            for iters in ITERS:
                for mu in MUS:
                    # the columns of a value row do not see each other: one restatement run serves the three device calls
                    w = want.smooth(np.concatenate([v, a1[:, None], a4], axis=1), iters=iters, mu=mu)
                    for layout in ("rows", "planes"):
                        got.layout = layout
                        what = (name, weights, boundary, iters, mu, layout)
                        assert same(got.smooth(iters=iters, mu=mu), np.ascontiguousarray(w[:, :3])), what
                        assert same(got.smooth(a1, iters=iters, mu=mu), np.ascontiguousarray(w[:, 3])), what
                        assert same(got.smooth(a4, iters=iters, mu=mu), np.ascontiguousarray(w[:, 4:])), what
            moved = want.smooth(iters=3)                     # normals of moved vertices over the same lists
            assert same(got.vertex_normals(moved, sign=-1.0), want.vertex_normals(moved, sign=-1.0)), (name, weights, boundary)


@pytest.mark.parametrize("name", ["icosphere_3", "lattice_33x33", "bipyramid_hub_last", "coincident_vertices", "obtuse", "isolated_vertices"])
def test_float32_is_widened_exactly_and_comes_back_float32(name):
    v, f = CASES[name]
    v32 = v.astype(np.float32)
    a1, a4 = attributes(v, np.float32)
    for weights in WEIGHTS:
        want = SN.Laplacian(v32, f, weights)
        got = mesh.MeshLaplacian(torch.from_numpy(v32).cuda(), torch.from_numpy(f).cuda(), weights)
        for iters in ITERS:
            s = got.smooth(iters=iters)
            assert s.dtype == torch.float32 and same(s, want.smooth(iters=iters)), (name, weights, iters)
            assert same(got.smooth(torch.from_numpy(a4).cuda(), iters=iters), want.smooth(a4, iters=iters)), (name, weights, iters)
            assert same(got.smooth(a1, iters=iters, lam=0.33, mu=-0.34), want.smooth(a1, iters=iters, lam=0.33, mu=-0.34)), (name, weights, iters)
        assert same(got.vertex_normals(sign=-1.0), want.vertex_normals(sign=-1.0)), (name, weights)
    assert same(mesh.smooth(v32, f, 0), v32)                 # iters = 0 returns the input's bits


def test_int64_faces_and_host_arrays_are_accepted():
    v, f = CASES["lattice_33x33"]
    want = SN.smooth(v, f, 3)
    assert same(mesh.smooth(torch.from_numpy(v), torch.from_numpy(f.astype(np.int64)).cuda(), 3), want)
    assert same(mesh.smooth(v, f.astype(np.int64), iters=3), want)
    assert same(mesh.vertex_normals(v, torch.from_numpy(f.astype(np.int64)), sign=-1.0), SN.vertex_normals(v, f, -1.0))
    sv, sn = mesh.smooth_with_normals(v, f, 3, weights="cotangent", boundary="free")
    L = SN.Laplacian(v, f, "cotangent", "free")
    assert same(sv, L.smooth(iters=3)) and same(sn, L.vertex_normals(L.smooth(iters=3), -1.0))


@pytest.mark.parametrize("name", ["icosphere_3", "lattice_33x33", "bipyramid_hub_last"])
def test_the_same_call_twice_gives_the_same_bits(name):
    v, f = CASES[name]
    for weights in WEIGHTS:
        a, b = mesh.smooth(v, f, 5, weights=weights), mesh.smooth(v, f, 5, weights=weights)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        L = mesh.MeshLaplacian(v, f, weights)
        assert torch.equal(L.smooth(iters=5).view(torch.int64), a.view(torch.int64))
        assert torch.equal(L.smooth(iters=5).view(torch.int64), a.view(torch.int64))      # the prepared mesh is not used up
        assert torch.equal(L.vertex_normals().view(torch.int64), mesh.vertex_normals(v, f).view(torch.int64))


REFUSED = {
    "a NaN coordinate": lambda v, f: (np.where(np.arange(v.size).reshape(v.shape) == 3 * 700 + 1, np.nan, v), f),
    "an infinite coordinate": lambda v, f: (np.where(np.arange(v.size).reshape(v.shape) == 5, np.inf, v), f),
    "a face index of V": lambda v, f: (v, np.concatenate([f[:1500], [[0, 1, len(v)]], f[1500:]]).astype(np.int32)),
    "a negative face index": lambda v, f: (v, np.concatenate([f, [[0, -1, 2]]]).astype(np.int32)),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_the_device_refuses_without_a_fault(what):
    v, f = CASES["lattice_33x33"]
    bv, bf = REFUSED[what](v, f)
    for weights in WEIGHTS:
        with pytest.raises(ValueError, match="dfh_mesh_smooth_prepare"):
            mesh.MeshLaplacian(bv, bf, weights)
        with pytest.raises(ValueError):
            SN.Laplacian(bv, bf, weights)
    assert same(mesh.smooth(v, f, 1), SN.smooth(v, f, 1))    # after a refusal


def test_python_refuses_what_the_library_would():
    v, f = CASES["tetrahedron"]
    L = mesh.MeshLaplacian(v, f)
    for kw in (dict(iters=-1), dict(lam=float("nan")), dict(mu=float("inf")), dict(lam=0.0), dict(x=np.zeros((4, 5))), dict(x=np.zeros((3, 3))),
               dict(x=np.zeros((4, 3), dtype=np.int32))):
        with pytest.raises(ValueError):
            L.smooth(**kw)
    with pytest.raises(ValueError):
        L.vertex_normals(sign=float("nan"))
    assert same(L.smooth(iters=2), SN.smooth(v, f, 2))


def test_taubin_keeps_the_sphere_that_laplace_shrinks():
    """The figures of tests/golden/smooth_recovery.json (tests/test_smooth_np.py states the three bounds) from the device's bits."""
    noisy, f = noisy_icosphere()
    rec = SN.golden_record(noisy, f, CENTRE, RADIUS, smoother=lambda *a, **kw: mesh.smooth(*a, **kw).cpu().numpy())
    print(json.dumps(rec, indent=1))
    assert rec["rms_radial_deviation_after_taubin"] <= 0.5 * rec["rms_radial_deviation_before"]
    assert abs(rec["mean_radius_shift_taubin"]) <= 0.05
    assert abs(rec["mean_radius_shift_laplace"]) > 0.5
    assert rec == json.load(open(os.path.join(GOLDEN, "smooth_recovery.json")))


def test_the_stored_marching_cubes_mesh_normals_and_fixed_boundary():
    d = np.load(os.path.join(GOLDEN, "g9_mesh.npz"))
    v, f, n = d["verts"], d["faces"], d["normals"]
    got = mesh.vertex_normals(v, f, sign=-1.0)
    assert got.dtype == torch.float32
    dots = (got.double().cpu().numpy() * n.astype(np.float64)).sum(axis=1)
    assert (dots > 0).all()                                  # marching-cubes normals point against the winding's right-hand normal
    L = mesh.MeshLaplacian(v, f)
    flagged = L.boundary.cpu().numpy()
    assert int(flagged.sum()) == 516
    moved = L.smooth(iters=10).cpu().numpy()
    assert np.array_equal(raw(moved[flagged]), raw(v[flagged])) and (moved[~flagged] != v[~flagged]).any(axis=1).mean() > 0.9
    free = mesh.smooth(v, f, 10, boundary="free").cpu().numpy()
    assert (free[flagged] != v[flagged]).any(axis=1).mean() > 0.9


# ---- the hooks, on an analytic sphere at 32^3 ---------------------------------------------------------------------------------
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
def test_write_canonical_mesh_writes_the_smoothed_mesh_and_leaves_the_stored_one(cls, tmp_path):
    fu = make(cls, sphere_volume())
    fu.marching_cubes()
    v0, f0 = fu._vertices.copy(), fu._faces.copy()
    assert fu.smooth_iters is None
    fu.write_canonical_mesh(str(tmp_path), "plain.obj")      # before the attribute is touched
    mv, mf, mn = fu._canonical_mesh_device()                 # the calls the method issued before it had the hook
    fu._write_mesh(str(tmp_path / "parent.obj"), mv.cpu().numpy(), mf.cpu().numpy(), mn.cpu().numpy(), None, None)
    assert open(tmp_path / "plain.obj", "rb").read() == open(tmp_path / "parent.obj", "rb").read()
    fu.smooth_iters = 2
    fu.write_canonical_mesh(str(tmp_path), "smooth.obj")
    assert np.array_equal(fu._vertices, v0) and np.array_equal(fu._faces, f0)
    fu.smooth_iters = None
    fu.write_canonical_mesh(str(tmp_path), "again.obj")
    assert open(tmp_path / "plain.obj", "rb").read() == open(tmp_path / "again.obj", "rb").read()
    sv = mesh.smooth(mv, mf, 2)                              # what the file must hold
    sn = mesh.vertex_normals(sv, mf, sign=-1.0)
    assert not torch.equal(sv, mv)
    fu._write_mesh(str(tmp_path / "want.obj"), sv.cpu().numpy(), mf.cpu().numpy(), sn.cpu().numpy(), None, None)
    assert open(tmp_path / "smooth.obj", "rb").read() == open(tmp_path / "want.obj", "rb").read()
    pv, pf, pn = mesh.read_obj(str(tmp_path / "plain.obj"))
    qv, qf, qn = mesh.read_obj(str(tmp_path / "smooth.obj"))
    assert np.array_equal(np.asarray(pf), np.asarray(qf)) and len(qv) == len(pv) == len(qn)
    length = np.linalg.norm(np.asarray(qn, dtype=np.float64), axis=1)
    assert (np.abs(length - 1.0) < 1e-5).all()               # unit, to the six decimals of the file
    assert ((np.asarray(qn, dtype=np.float64) * np.asarray(pn, dtype=np.float64)).sum(axis=1) > 0.9).all()


def test_colored_mesh_smooths_before_it_samples_the_colours():
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
    v1, f1, n1, rgb1, ok1 = sf.colored_mesh(smooth_iters=2)
    sv, sn = mesh.smooth_with_normals(wv, wf, 2)
    assert torch.equal(v1, sv) and torch.equal(f1, wf) and torch.equal(n1, sn) and not torch.equal(v1, v0)
    assert torch.equal(sv, mesh.smooth(wv, wf, 2)) and torch.equal(sn, mesh.vertex_normals(sv, wf, sign=-1.0))
    rgb, ok = kernels.sample_colors(sf.C, v1.double())       # the colour volume at the moved vertices
    assert torch.equal(ok1, ok) and torch.equal(rgb1[ok1], rgb[ok]) and bool(ok1.any())
    length = torch.linalg.vector_norm(n1.double(), dim=1)
    assert bool(((length - 1.0).abs() < 1e-6).all())
    v2, f2, n2, _, _ = sf.colored_mesh(simplify_cell=2.0, smooth_iters=2)       # smoothing first, then the simplification
    cv, cf, cn, _ = mesh.simplify_with_normals(sv, wf, sn, 2.0)
    assert torch.equal(v2, cv) and torch.equal(f2, cf) and torch.equal(n2, cn)
