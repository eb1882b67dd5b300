"""CPU: the K22 restatement (tests/mesh_sdf_np.py) against hand-derived and analytic answers, and mesh.pseudonormals against
the restatement's loop-written tables."""
import numpy as np
import pytest

import mesh_sdf_cases as MC
import mesh_sdf_np as MN
from dynamicfusion_body_amd import mesh


def test_one_triangle_all_seven_regions():
    """A = (0,0,0), B = (2,0,0), C = (0,2,0); every point at height 1 above its hand-derived closest point."""
    A, B, C = np.array([0.0, 0, 0]), np.array([2.0, 0, 0]), np.array([0.0, 2, 0])
    P = np.array([[-1, -1, 1], [3, -0.5, 1], [-0.5, 3, 1], [1, -1, 1], [-1, 1, 1], [2, 2, 1], [0.5, 0.5, 1]], dtype=np.float64)
    Q, feat, D2 = MN.closest_on_face(P, A, B, C)
    assert feat.tolist() == [0, 1, 2, 3, 4, 5, 6]
    want = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0]], dtype=np.float64)
    assert np.array_equal(Q, want)
    assert np.array_equal(D2, ((P - want) ** 2).sum(1))
    val, closest, face, known, _ = MN.query(P, np.stack([A, B, C]), [[0, 1, 2]])
    assert known.all() and (face == 0).all() and np.array_equal(val, np.sqrt(D2))          # above a face wound towards +z: outside
    val, _, _, _, _ = MN.query(P * [1, 1, -1], np.stack([A, B, C]), [[0, 1, 2]])
    assert np.array_equal(val, -np.sqrt(D2))


@pytest.fixture(scope="module")
def l_case():
    v, f = MC.l_prism()
    assert len(f) == 20
    P = MN.grid_points(**MC.L_GRID)
    return v, f, P, MC.l_inside(P).reshape(MC.L_GRID["shape"])


def test_l_prism_sign_is_the_analytic_one_everywhere(l_case):
    v, f, P, inside = l_case
    vol, _, _, known = MN.grid(v, f, band=np.inf, dtype=np.float64, **MC.L_GRID)
    assert known.all() and (vol != 0).all()
    assert int(((vol < 0) != inside).sum()) == 0 and vol.size == 5832


def test_l_prism_values_do_not_depend_on_the_face_order(l_case):
    v, f, P, _ = l_case
    perm = np.random.RandomState(3).permutation(len(f))
    a = MN.query(P, v, f)
    b = MN.query(P, v, f[perm])
    assert a[0].tobytes() == b[0].tobytes()           # (the closest POINT may move between equidistant faces: the index breaks ties)


def test_l_prism_far_fill_is_the_analytic_sign(l_case):
    v, f, P, inside = l_case
    vol, _, face, known = MN.grid(v, f, band=1.0, dtype=np.float64, **MC.L_GRID)
    assert not known.all() and (face[~known] == -1).all() and (np.abs(vol[~known]) == 1.0).all()
    assert int(((vol < 0) != inside).sum()) == 0


def test_cube_ties_pick_the_lowest_face_and_the_surface_is_plus_zero():
    v, f = MC.cube(0.0, 4.0)
    P = MN.grid_points(-2.0, 1.0, (9, 9, 9))
    val, closest, face, known, _ = MN.query(P, v, f)
    on = (MC.box_distance(P, 0.0, 4.0) == 0) & (((P == 0) | (P == 4)).any(1))
    assert on.sum() == 5 ** 3 - 3 ** 3
    assert (val[on] == 0).all() and not np.signbit(val[on]).any()
    # every face that attains the minimum, by brute force: the reported one is the lowest
    D2 = np.stack([MN.closest_on_face(P, v[a], v[b], v[c])[2] for a, b, c in f], axis=1)
    assert np.array_equal(face, np.argmax(D2 == D2.min(1, keepdims=True), axis=1))
    assert ((D2 == D2.min(1, keepdims=True)).sum(1) > 1).sum() > 300                      # the lattice is full of exact ties
    inside = ((P > 0) & (P < 4)).all(1)
    assert ((val < 0) == inside).all()


def test_cube_distance_is_the_box_formula_outside():
    v, f = MC.cube(0.0, 4.0)
    P = np.random.RandomState(11).uniform(-5, 9, (4000, 3))
    P = P[~((P >= 0) & (P <= 4)).all(1)]
    val = MN.query(P, v, f)[0]
    assert np.abs(val - MC.box_distance(P, 0.0, 4.0)).max() <= 1e-12


def tables_mesh():
    """A tetrahedron with one face missing (three boundary edges), a fin on an edge (non-manifold: three sharers), a zero-area
    face, and a face that repeats a vertex."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [0.5, 0, 0]], dtype=np.float64)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [0, 1, 4], [0, 5, 1], [2, 2, 3]], dtype=np.int32)
    return v, f


@pytest.mark.parametrize("which", ["tables_mesh", "l_prism", "icosphere", "float32"])
def test_pseudonormals_equal_the_loop_version_bit_for_bit(which):
    v, f = {"tables_mesh": tables_mesh, "l_prism": MC.l_prism, "icosphere": lambda: MC.icosphere(1, 3.0, 1.0),
            "float32": lambda: (MC.icosphere(1, 3.0, 1.0)[0].astype(np.float32), MC.icosphere(1)[1])}[which]()
    got = mesh.pseudonormals(v, f)
    want = MN.pseudonormals_loops(v, f)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert g.tobytes() == w.tobytes()
    if which == "tables_mesh":
        fn, en, vn, dropped = got
        assert dropped.tolist() == [False, False, False, False, True, True]
        assert np.array_equal(en[0, 2], fn[0])                                            # edge (2, 1): boundary
        assert np.array_equal(en[0, 1], (fn[0] + fn[1]) + fn[3])                          # edge (0, 1): three sharers, ascending
        assert np.array_equal(en[1, 0], en[0, 1]) and np.array_equal(en[3, 0], en[0, 1])
        assert not fn[4].any() and not en[4].any() and not vn[5].any()


def test_pseudonormals_refuse_bad_meshes():
    v, f = tables_mesh()
    with pytest.raises(ValueError):
        mesh.pseudonormals(v, np.array([[0, 1, 6]]))
    with pytest.raises(ValueError):
        mesh.pseudonormals(v, f.astype(np.float64))
    with pytest.raises(ValueError):
        mesh.pseudonormals(v[:, :2], f)


def test_the_banded_restatement_is_the_plain_one(l_case):
    """mesh_sdf_np.grid_banded (each face only at the vertices within band + a spacing of its box: what makes g9's 65^3 feasible in
    numpy) gives grid()'s volume, closest points, faces and known flags."""
    v, f, _, _ = l_case
    a = MN.grid(v, f, band=1.0, **MC.L_GRID)
    b = MN.grid_banded(v, f, band=1.0, **MC.L_GRID)
    assert [x.tobytes() == y.tobytes() for x, y in zip(a, b)] == [True] * 4
