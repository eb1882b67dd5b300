"""GPU: K23, mesh connected components (csrc/dfh_mesh_components.hip) against tests/components_np.py, bit for bit on every output:
labels, ids, the per-component table (counts, box, area in the stated order) and the compaction, at the shapes where they can
go wrong (tests/components_cases.py), then through mesh.filter_components and the Fusion / FusionDM / colored_mesh hooks."""
import os

import numpy as np
import pytest
import torch

import components_np as CN
from components_cases import CASES, KEEP_MASKS, keep_mask
from dynamicfusion_body_amd import Fusion, FusionDM, mesh

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INT_FIELDS = ("vert_root", "vert_comp", "face_comp", "root", "n_verts", "n_faces")


@pytest.fixture(scope="module")
def restated():
    """The numpy restatement of every case, computed once (float64 vertices) and left alone."""
    return {name: CN.components(v, f) for name, (v, f) in CASES.items()}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_components_equal(got, want, what):
    assert got.n == want["n"], what
    for k in INT_FIELDS:
        g = getattr(got, k).cpu().numpy()
        assert g.dtype == np.int32 and np.array_equal(g, want[k]), (what, k)
    for k in ("bbox_min", "bbox_max"):                      # a NaN entry has the header's bits
        assert np.array_equal(bits(getattr(got, k).cpu().numpy()), bits(want[k])), (what, k)
    a, b = got.area.cpu().numpy(), want["area"]
    nan = np.isnan(b)                                        # (an area that is a NaN is a NaN: its payload is nobody's promise)
    assert np.array_equal(np.isnan(a), nan) and np.array_equal(bits(a)[~nan], bits(b)[~nan]), (what, "area")


@pytest.mark.parametrize("name", sorted(CASES))
def test_labels_and_table_equal_the_restatement(restated, name):
    v, f = CASES[name]
    assert_components_equal(mesh.connected_components(v, f), restated[name], name)


@pytest.mark.parametrize("name", ["soup_257", "isolated_3000", "fan_hub_last", "degenerate_duplicate_unreferenced", "strip_F1025"])
def test_float32_vertices_are_widened_exactly(name):
    v, f = CASES[name]
    v32 = v.astype(np.float32)
    got = mesh.connected_components(torch.from_numpy(v32).cuda(), torch.from_numpy(f).cuda())
    assert_components_equal(got, CN.components(v32, f), name)


@pytest.mark.parametrize("name", ["strip_permuted", "fan_hub_last", "isolated_3000", "soup_1025"])
def test_the_same_case_twice_gives_the_same_bits(name):
    v, f = CASES[name]
    a, b = mesh.connected_components(v, f), mesh.connected_components(v, f)
    for k in INT_FIELDS + ("area", "bbox_min", "bbox_max"):
        assert torch.equal(getattr(a, k).view(torch.int64) if getattr(a, k).dtype == torch.float64 else getattr(a, k),
                           getattr(b, k).view(torch.int64) if getattr(b, k).dtype == torch.float64 else getattr(b, k)), k
    ka = torch.from_numpy(keep_mask("alternating", a.n)).cuda()
    for x, y in zip(mesh.compact_components(a, ka), mesh.compact_components(b, ka)):
        assert torch.equal(x, y)


def test_int64_faces_and_tensors_are_accepted(restated):
    v, f = CASES["soup_1023"]
    got = mesh.connected_components(torch.from_numpy(v).cuda(), torch.from_numpy(f.astype(np.int64)).cuda())
    assert_components_equal(got, restated["soup_1023"], "int64 faces")


def test_a_nan_coordinate_stays_in_its_component(restated):
    v, f = CASES["isolated_3000"]
    want = restated["isolated_3000"]
    vn = v.copy()
    vn[3 * 1500 + 1, 2] = np.nan                            # component 1500, in the middle of a scan chunk
    vn[3 * 2999, 0] = np.inf                                # and an infinity in the last one
    got = mesh.connected_components(vn, f)
    assert_components_equal(got, CN.components(vn, f), "nan")
    for k in INT_FIELDS:                                    # labels and counts read no coordinate
        assert np.array_equal(getattr(got, k).cpu().numpy(), want[k]), k
    others = np.ones(3000, dtype=bool)
    others[[1500, 2999]] = False
    for k in ("area", "bbox_min", "bbox_max"):
        assert np.array_equal(bits(getattr(got, k).cpu().numpy())[others], bits(want[k])[others]), k
    assert np.isnan(got.area[1500].item()) and np.isnan(got.bbox_min[1500, 2].item()) and np.isnan(got.bbox_max[1500, 2].item())
    assert got.bbox_max[2999, 0].item() == np.inf and np.isfinite(got.bbox_min[1500, :2].cpu().numpy()).all()


@pytest.mark.parametrize("bad", [("index == V", 0), ("index negative", -1)])
def test_a_bad_index_is_refused_and_touches_nothing(restated, bad):
    what, delta = bad
    v, f = CASES["soup_1025"]
    before = mesh.connected_components(v, f)
    guard = torch.full((4096,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")     # neighbours on the heap: must stay as they are
    fb = f.copy()
    fb[513, 1] = len(v) if delta == 0 else -1
    with pytest.raises(ValueError, match="dfh_mesh_components"):
        mesh.connected_components(v, fb)
    torch.cuda.synchronize()
    assert bool((guard == 0x5A5A5A5A).all())
    assert_components_equal(before, restated["soup_1025"], "the call before")
    assert_components_equal(mesh.connected_components(v, f), restated["soup_1025"], "the call after")
    # compaction refuses what does not belong together too: labels of another mesh (component ids outside [0, C))
    stale = mesh.connected_components(*CASES["isolated_3000"])
    stale.n = 5
    with pytest.raises(ValueError, match="dfh_mesh_compact"):
        mesh.compact_components(stale, np.ones(5, dtype=np.uint8))
    torch.cuda.synchronize()


COMPACT_CASES = ["no_vertices", "no_faces_5_verts", "one_face", "two_disjoint_faces", "degenerate_duplicate_unreferenced", "isolated_3000",
                 "isolated_V1025", "soup_255", "soup_256", "soup_257", "soup_1023", "soup_1024", "soup_1025", "strip_F1024", "fan_hub_last"]


@pytest.mark.parametrize("name", COMPACT_CASES)
def test_compaction_equals_the_restatement(restated, name):
    v, f = CASES[name]
    comps = mesh.connected_components(v, f)
    want = restated[name]
    for kind in KEEP_MASKS:
        keep = keep_mask(kind, want["n"])
        for drop in (True, False):
            kept, vmap, f2 = (t.cpu().numpy() for t in mesh.compact_components(comps, keep, drop_unreferenced=drop))
            wk, wm, wf = CN.compact(f, want["vert_comp"], want["face_comp"], keep, drop)
            assert kept.dtype == vmap.dtype == f2.dtype == np.int32
            assert np.array_equal(kept, wk) and np.array_equal(vmap, wm) and np.array_equal(f2, wf), (name, kind, drop)


def test_filter_components_gathers_attributes(restated):
    v, f = CASES["soup_1025"]
    want = restated["soup_1025"]
    normals = np.random.default_rng(3).normal(size=v.shape).astype(np.float32)
    colour = np.arange(len(v), dtype=np.int64)
    for kw in (dict(min_faces=3), dict(min_area=2.0), dict(keep_largest=2), dict(keep_largest=3, min_faces=2, drop_unreferenced=False), dict()):
        drop = kw.get("drop_unreferenced", True)
        keep = CN.keep_mask(want, kw.get("min_faces", 0), kw.get("min_area", 0.0), kw.get("keep_largest"))
        wk, _, wf = CN.compact(f, want["vert_comp"], want["face_comp"], keep, drop)
        v2, f2, n2, c2, idx = mesh.filter_components(v, f, normals, torch.from_numpy(colour), **kw)
        assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), wk) and np.array_equal(f2.cpu().numpy(), wf), kw
        assert np.array_equal(v2.cpu().numpy(), v[wk]) and np.array_equal(n2.cpu().numpy(), normals[wk]) and np.array_equal(c2.cpu().numpy(), colour[wk])
    with pytest.raises(ValueError):
        mesh.filter_components(v, f, normals[:-1])


def test_keep_largest_ties_go_to_the_lower_id():
    v, f = CASES["isolated_3000"]                           # 3000 components of one face each
    _, f2, idx = mesh.filter_components(v, f, keep_largest=2)
    assert idx.tolist() == [0, 1, 2, 3, 4, 5] and f2.tolist() == [[0, 1, 2], [3, 4, 5]]


def test_g9_mesh_is_one_component_and_survives_unchanged():
    d = np.load(os.path.join(GOLDEN, "g9_mesh.npz"))
    v, f = d["verts"], d["faces"].astype(np.int32)
    c = mesh.connected_components(v, f)
    assert c.n == 1 and c.n_verts.tolist() == [16741] and c.n_faces.tolist() == [32970] and c.root.tolist() == [0]
    assert_components_equal(c, CN.components(v, f), "g9")
    v2, f2, idx = mesh.filter_components(v, f, keep_largest=1)
    assert np.array_equal(v2.cpu().numpy(), v) and np.array_equal(f2.cpu().numpy(), f) and np.array_equal(idx.cpu().numpy(), np.arange(len(v)))


# ---- end to end at 32^3: two spheres of different size and a blob of about three voxels ------------------------------------------
BLOB_C, BLOB_LO, BLOB_HI = (26.3, 6.4, 6.2), np.array([23.0, 3.0, 3.0]), np.array([30.0, 10.0, 10.0])


def scene_volume():
    g = np.stack(np.meshgrid(*[np.arange(32.0)] * 3, indexing="ij"), axis=-1)
    d = lambda c, r: np.linalg.norm(g - np.asarray(c), axis=-1) - r
    sd = np.minimum(np.minimum(d((10.2, 10.4, 10.1), 6.3), d((21.7, 22.1, 20.3), 4.2)), d(BLOB_C, 0.9))
    return np.clip(sd, -3.0, 3.0).astype(np.float32)


def in_blob_box(p):
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return ((p >= BLOB_LO) & (p <= BLOB_HI)).all(axis=1)


def test_marching_cubes_of_two_spheres_and_a_blob_has_three_components():
    T = torch.from_numpy(scene_volume()).cuda()
    v, f, n, val = mesh.marching_cubes(T, 0.0)
    c = mesh.connected_components(v, f)
    assert c.n == 3
    assert_components_equal(c, CN.components(v.cpu().numpy(), f.cpu().numpy()), "scene")
    blob = int(torch.argmin(c.n_faces))
    assert 0 < int(c.n_faces[blob]) < 60 and in_blob_box(c.bbox_min[blob].cpu().numpy())[0] and in_blob_box(c.bbox_max[blob].cpu().numpy())[0]
    v2, f2, n2, idx = mesh.filter_components(v, f, n, min_faces=60)
    assert len(v2) == len(v) - int(c.n_verts[blob]) and len(f2) == len(f) - int(c.n_faces[blob])
    assert not in_blob_box(v2.cpu().numpy()).any() and in_blob_box(v.cpu().numpy()).any()
    assert torch.equal(n2, n[idx]) and mesh.connected_components(v2, f2).n == 2


@pytest.mark.parametrize("cls", ["Fusion", "FusionDM"])
def test_min_component_faces_cleans_the_stored_mesh_and_the_graph(cls):
    vol = scene_volume()

    def make():
        if cls == "Fusion":
            return Fusion(vol.copy(), 3.0, subsample_rate=2.0, knn=4, marching_cubes_step_size=1, write_warpfield=False)
        fu = FusionDM(3.0, np.array([[100.0, 0, 16], [0, 100.0, 16], [0, 0, 1]]), tsdf_res=32, marching_cubes_step_size=1, write_warpfield=False)
        fu._ensure_volumes()
        fu._T.copy_(torch.from_numpy(vol))
        return fu

    T = torch.from_numpy(vol).cuda()
    v0, f0, n0, _ = mesh.marching_cubes(T, None, 1, as_numpy=True)
    plain = make()
    assert plain.min_component_faces is None
    plain.marching_cubes()                                   # the attribute left at None: the mesh as it always was, bit for bit
    assert np.array_equal(plain._vertices, v0) and np.array_equal(plain._faces, f0) and np.array_equal(plain._normals, n0)
    assert in_blob_box(plain._vertices).any()
    clean = make()
    clean.min_component_faces = 60
    clean.marching_cubes()
    assert not in_blob_box(clean._vertices).any() and len(clean._vertices) < len(v0) and len(clean._faces) < len(f0)
    assert len(clean._normals) == len(clean._vertices) and clean._faces.max() == len(clean._vertices) - 1
    wv, wf, wn, _ = mesh.filter_components(v0, f0, n0, min_faces=60)
    assert np.array_equal(clean._vertices, wv.cpu().numpy()) and np.array_equal(clean._faces, wf.cpu().numpy())
    assert np.array_equal(clean._normals, wn.cpu().numpy())
    if cls == "Fusion":
        plain.initialize_canonical()
        clean.initialize_canonical()
        assert in_blob_box([nd[1] for nd in plain._nodes]).any()          # today a node sits on the blob
        assert len(clean._nodes) >= 4 and not in_blob_box([nd[1] for nd in clean._nodes]).any()
        assert not in_blob_box(clean._vertices).any()


def test_colored_mesh_drops_the_fragments_on_request():
    """SlabFrame.colored_mesh reads the frame's T, C and rank count only: a bare frame with the scene's volume and a colour volume
    that is one colour everywhere.  Default: the mesh of today, blob included; min_component_faces: the mesh without it, colours
    sampled at the surviving vertices."""
    from dynamicfusion_body_amd import kernels
    from dynamicfusion_body_amd.pipeline import SlabFrame
    sf = SlabFrame.__new__(SlabFrame)
    sf.ws = 1
    sf.T = torch.from_numpy(scene_volume()).cuda()
    sf.C = kernels.color_volume((32, 32, 32))
    sf.C[..., 0], sf.C[..., 1], sf.C[..., 2], sf.C[..., 3] = 10.0, 20.0, 30.0, 1.0
    v0, f0, n0, rgb0, ok0 = sf.colored_mesh()
    wv, wf, wn, _ = mesh.marching_cubes(sf.T, 0.0, 1)
    assert torch.equal(v0, wv) and torch.equal(f0, wf) and torch.equal(n0, wn) and in_blob_box(v0.cpu().numpy()).any()
    v1, f1, n1, rgb1, ok1 = sf.colored_mesh(min_component_faces=60)
    cv, cf, cn, _ = mesh.filter_components(wv, wf, wn, min_faces=60)
    assert torch.equal(v1, cv) and torch.equal(f1, cf) and torch.equal(n1, cn) and not in_blob_box(v1.cpu().numpy()).any()
    assert rgb1.shape == v1.shape and ok1.shape == (len(v1),) and bool(ok1.all())
    assert torch.equal(rgb1[ok1], torch.tensor([10.0, 20.0, 30.0], device="cuda").expand(int(ok1.sum()), 3))
