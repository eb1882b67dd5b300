"""CPU: the K20 restatement (tests/raycast_np.py) against analytic scenes and K1's oracle, and the properties of the walk the GPU
tests then hold the device to bit for bit.  No GPU, no library call."""
import json
import math
import os

import numpy as np
import pytest

import raycast_cases as RC
import raycast_np as RN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raycast_recovery.json")


def sphere_figures():
    """The analytic sphere (32^3, r = 10, three cameras): |z* - z_true| in voxels over the rays that hit at more than 30 degrees
    from grazing, and the angle between the cast and the analytic normal over the same rays."""
    c = RC.cases()["sphere_f32_3views"]
    e = c.expected()
    errs, angs = [], []
    for v, (z, cosang, L, ncam) in enumerate(RC.sphere_truth(c, (16.3, 15.6, 15.9), 10.0)):
        m = (e["depth"][v] != 0) & (cosang > 0.5)
        errs.append(np.abs(-e["depth"][v][m].astype(np.float64) - z[m]) * L[m])
        n = e["normals"][v][m].astype(np.float64)
        assert np.all(np.abs(np.linalg.norm(n, axis=-1) - 1.0) < 1e-6)
        angs.append(np.arccos(np.clip(np.sum(n * ncam[m], axis=-1), -1.0, 1.0)))
    errs, angs = np.concatenate(errs), np.concatenate(angs)
    return {"rays": int(errs.size), "mean_abs_dz_vox": float(errs.mean()), "max_abs_dz_vox": float(errs.max()),
            "median_normal_angle_rad": float(np.median(angs))}


def roundtrip_figures():
    c, depths = RC.roundtrip()
    e = RN.raycast(c.T, c.Wt, c.Kinv, c.wls, c.H, c.W, c.scale, c.center, half=c.tsdf_res / 2.0, **c.kw)
    med, p95, n = RC.roundtrip_figures(e["depth"], depths)
    return {"pixels": n, "median_abs_diff": med, "p95_abs_diff": p95}


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _same(got, want):
    for k, v in want.items():
        if isinstance(v, int):
            assert got[k] == v, (k, got[k], v)
        else:
            assert got[k] == pytest.approx(v, rel=1e-6), (k, got[k], v)


def test_sphere_recovery():
    """Trilinear interpolation of a function with Hessian norm <= 2 / rho is off by at most 2 h^2 / (8 rho) = 0.025 voxel at
    rho = 10 and the secant root adds second-order error: the mean must stay below twice that.  The normal must be closer to the
    analytic one than the angle one voxel subtends at radius r."""
    f = sphere_figures()
    print(f)
    assert f["rays"] > 500
    assert f["mean_abs_dz_vox"] <= 0.05
    assert f["median_normal_angle_rad"] < math.asin(1.0 / 10.0)
    _same(f, _golden()["sphere"])


def test_roundtrip_with_k1_oracle():
    """Depth maps fused by oracle_np.fuse_depths and cast back from the same cameras: the figures are recorded, not bounded (the
    GPU test asserts that the device reproduces them)."""
    f = roundtrip_figures()
    print(f)
    assert f["pixels"] > 1000
    _same(f, _golden()["roundtrip"])


def test_no_tie_class_in_any_scene():
    for name, c in RC.cases().items():
        assert c.expected()["excluded"] == 0, name


def test_zero_direction_components_are_exact():
    c = RC.cases()["dyadic_sphere"]
    wl = c.wls[0]
    rho = c.Kinv @ np.array([4.0, 4.0, 1.0])
    assert np.array_equal(wl[:, :3] @ rho, np.array([0.0, 0.0, 1.0]))
    e = c.expected()
    assert e["depth"][0, 4, 4] != 0
    assert e["hit"][0, 4, 4, 0] == 12.0 and e["hit"][0, 4, 4, 1] == 12.0             # the ray never leaves its column


def test_lattice_zeros_are_crossings():
    """Integer-plane SDF, axis-aligned camera, step 1: the central ray's samples land on voxels, one of them on T == 0 exactly; t <= 0
    makes it the crossing and the secant root is that sample."""
    c = RC.cases()["lattice_zeros_step1"]
    e = c.expected()
    assert np.all(e["depth"] != 0)
    assert e["hit"][0, 4, 4, 2] == 10.0
    assert e["samples"][0, 4, 4] == 9                                              # i_2 = 2 .. 10


def test_unknown_gap_hides_a_crossing():
    e1, e0 = RC.cases()["gap_min_weight_1"].expected(), RC.cases()["gap_min_weight_0"].expected()
    assert not np.any(e1["depth"] != 0) and np.all(np.isnan(e1["hit"]))
    assert np.all(e0["depth"] != 0)


def test_minus_to_plus_is_never_a_hit():
    e = RC.cases()["minus_to_plus"].expected()
    assert not np.any(e["depth"] != 0)
    assert np.all(e["samples"] == e["steps"])                                      # every ray walked to its end


def test_camera_inside_the_surface_sees_free_space_first():
    c = RC.cases()["camera_inside_surface"]
    e = c.expected()
    assert np.all(e["depth"] != 0)
    assert np.all(e["hit"][..., 2] > 30.0)                                         # the wall, not the sphere the camera sits in
    g = RN.Grid(c.T, c.Wt)
    o = (c.wls[0][:, 3] - c.center) / c.scale + c.tsdf_res / 2.0
    assert RN.value(g, o[:1], o[1:2], o[2:], 0.0)[1][0] < 0.0                      # the eye itself is behind the surface


def test_misses_and_cuts():
    assert np.any(RC.cases()["camera_inside_grid"].expected()["depth"] == 0)       # rays that miss the box
    e = RC.cases()["z_near_beyond_surface"].expected()
    hit = e["depth"] != 0
    assert hit.any() and np.all(-e["depth"][hit] >= RC.SCALE * 32.0)
    assert e["hit"][0, 8, 10, 2] > 30.0                        # z_near lies inside the sphere on the central rays: they see the wall
    e = RC.cases()["max_steps_10"].expected()
    assert not np.any(e["depth"] != 0) and e["steps"].max() == 11
    a, b = RC.cases()["refine_0"].expected(), RC.cases()["refine_8"].expected()
    assert np.array_equal(a["depth"] != 0, b["depth"] != 0) and not np.array_equal(a["depth"], b["depth"])


def test_slab_is_not_the_full_cast_restricted():
    """Rays of the slab cast equal the full-grid cast only where the restatement says so: the slab's own box clips them."""
    full, slab = RC.cases()["ragged_9x65"].expected(), RC.cases()["slab_5_12"].expected()
    both = (full["depth"] != 0) & (slab["depth"] != 0)
    assert both.any() and ((full["depth"] != 0) & (slab["depth"] == 0)).any()
    assert np.all((slab["hit"][..., 0][slab["depth"] != 0] >= 5.0) & (slab["hit"][..., 0][slab["depth"] != 0] <= 11.0))


def test_colour_rule():
    c = RC.cases()["colour"]
    e = c.expected()
    hit = e["depth"] != 0
    col = e["color"][..., 3] == 255
    assert col.any() and (hit & ~col).any() and not (col & ~hit).any()
    assert np.all(e["color"][~col] == 0)                                           # no coloured corner: 0, 0, 0, 0
    # painted by position: red = 7 i_0 + 3 is linear, so the trilinear mean over a fully coloured cell reproduces it
    v, y, x = [int(a[0]) for a in np.nonzero(col & (e["hit"][..., 1] > 17.0))]
    assert abs(int(e["color"][v, y, x, 0]) - (7.0 * float(e["hit"][v, y, x, 0]) + 3.0)) <= 1.0


def test_brick_table_restatement():
    t = RN.brick_table(RC.cases()["all_free"].T)
    assert t.shape == (3, 3, 3) and not t.any()
    t = RN.brick_table(RC.cases()["plane_at_8"].T)                                 # T = 8 - i_2: voxel 8 holds 0, brick 0's ring reaches it
    assert t.all()                                                                 # (behind the plane T < 0: live)
    t = RN.brick_table(RC.cases()["plane_at_16"].T)                                # T = 1 at voxel 15, 0 at 16: brick 0's ring ends at 9
    assert not t[:, :, 0].any() and t[:, :, 1].all() and t[:, :, 2].all()
    tiny = np.full((8, 8, 8), 1.0, dtype=np.float32)
    tiny[3, 3, 3] = 1e-12                                                          # > 0 but not safely: live
    assert RN.brick_table(tiny).all()
