"""CPU: the normal-compatibility gate of the depth data term -- what it buys, measured on the numpy restatement
(tests/assoc_normals_np.py), and what the four gated entry points do with arguments they cannot use (validation comes before any
HIP call: device pointers are dummy non-null integers, as in tests/test_abi_volume_fused.py)."""
import ctypes
import functools
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import assoc_normals_np as AN
import assoc_normals_scenes as SC
from dynamicfusion_body_amd import _lib, build
from oracle import gn_np as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "normal_gate_recovery.json")
MIN_COS = 0.5


def _both(sc, max_dist):
    """(corr, valid) without and with the gate, under the identity field."""
    cu, vu, _ = G.associate_depth_views(sc.pos, SC.K, SC.KINV, sc.lws, sc.dms, SC.SCALE, SC.CENTER, SC.HALF, max_dist)
    _, nw = AN.warped(sc.pos, sc.nrm, sc.dqs, sc.nbr, sc.node_pos, sc.node_w, SC.IDENT)
    cg, vg, _, edge = AN.associate_depth_views_gated(sc.pos, nw, SC.K, SC.KINV, sc.lws, sc.dms, sc.nmaps, SC.SCALE, SC.CENTER, SC.HALF,
                                                     max_dist, MIN_COS)
    assert not edge.any()
    return (cu, vu), (cg, vg)


def _row(sc, cv):
    c, v = cv
    return {"valid": int(v.sum()), "wrong_side": int(sc.wrong_side(c, v).sum()), "image_error": sc.image_error(c, v)}


def rigid_step(sc, gated, max_dist=4.5):
    """One rigid-mode step (gn_np.global_step_sampled, lm_rel 0.1, no Huber) -> (displacement of the ball's centre, valid count)."""
    def associate(wp):
        if not gated:
            c, v, _ = G.associate_depth_views(wp, SC.K, SC.KINV, sc.lws, sc.dms, SC.SCALE, SC.CENTER, SC.HALF, max_dist)
            return c, v
        _, nw = AN.warped(sc.pos, sc.nrm, sc.dqs, sc.nbr, sc.node_pos, sc.node_w, SC.IDENT)
        c, v, _, _ = AN.associate_depth_views_gated(wp, nw, SC.K, SC.KINV, sc.lws, sc.dms, sc.nmaps, SC.SCALE, SC.CENTER, SC.HALF, max_dist,
                                                    MIN_COS)
        return c, v
    dqs, _, count = G.global_step_sampled(sc.dqs, sc.pos, sc.nrm, sc.nbr, sc.node_pos, sc.node_w, SC.IDENT, associate, 0.0, 0.1)
    return SC.centre_displacement(dqs[0]), count


@pytest.fixture(scope="module")
def measured():
    one, two = SC.thin((0,)), SC.thin((0, 180))
    (u1, g1), (u2, g2) = _both(one, 4.5), _both(two, 3.0)
    du, _ = rigid_step(one, False)
    dg, _ = rigid_step(one, True)
    return {"one_view": {"ungated": _row(one, u1), "gated": _row(one, g1)},
            "two_views": {"ungated": _row(two, u2), "gated": _row(two, g2)},
            "rigid_step_dz": {"ungated": float(du[2]), "gated": float(dg[2]), "true": 1.5}}


def test_the_gate_removes_every_wrong_side_match_of_one_view(measured):
    u, g = measured["one_view"]["ungated"], measured["one_view"]["gated"]
    assert u["wrong_side"] > 500 and g["wrong_side"] == 0          # (589 -> 0)
    assert 0 < g["valid"] < u["valid"]
    assert g["image_error"] < 0.25 * u["image_error"]              # (1.26 -> 0.19 voxels)


def test_the_gate_removes_every_wrong_side_match_of_two_opposite_views(measured):
    u, g = measured["two_views"]["ungated"], measured["two_views"]["gated"]
    assert u["wrong_side"] > 50 and g["wrong_side"] == 0           # (84 -> 0)
    assert 0 < g["valid"] < u["valid"]
    assert g["image_error"] < 0.3 * u["image_error"]               # (0.70 -> 0.135 voxels)


def test_the_gated_rigid_step_recovers_the_motion_the_ungated_one_loses(measured):
    dz = measured["rigid_step_dz"]
    assert dz["gated"] > 1.0 and dz["ungated"] < 0.5               # true motion 1.5; the back-facing rows cancel the front-facing ones


def test_the_measurements_are_the_recorded_ones(measured):
    gold = json.load(open(GOLDEN))
    for scene_ in ("one_view", "two_views"):
        for variant in ("ungated", "gated"):
            m, g = measured[scene_][variant], gold[scene_][variant]
            assert abs(m["valid"] - g["valid"]) <= 3 and abs(m["wrong_side"] - g["wrong_side"]) <= 3, (scene_, variant, m, g)
            assert abs(m["image_error"] - g["image_error"]) <= 5e-3, (scene_, variant, m, g)
    for variant in ("ungated", "gated"):
        assert abs(measured["rigid_step_dz"][variant] - gold["rigid_step_dz"][variant]) <= 5e-3


def test_the_gate_on_the_ordinary_sphere_keeps_most_correspondences():
    sc = SC.ordinary(move=(0.0, 0.0, 0.0))
    (cu, vu), (cg, vg) = _both(sc, 2.0)
    assert 0.75 * vu.sum() < vg.sum() <= vu.sum()                  # (2 295 -> 1 913 at rest)
    assert not (vg & ~vu).any()                                    # the gate only removes
    assert sc.image_error(cg, vg) < sc.image_error(cu, vu)


# ------------------------------------------------------------------------------- the C ABI's argument checks
OK, BADARG = 0, -1
PTR = 0x1000
NAN, INF = float("nan"), float("inf")
BIG = 1 << 30


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.load()


def on_own_thread(test):
    """dfh_last_error() is kept per thread: the refused calls are made on a thread of their own."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        with ThreadPoolExecutor(1) as ex:
            return ex.submit(test, *args, **kwargs).result()
    return run


def problem(**over):
    p = _lib.Problem()
    for f, t in _lib.Problem._fields_:
        if t is ctypes.c_void_p:
            setattr(p, f, PTR)
    p.n_samples, p.knn, p.n_nodes, p.n_blocks, p.n_upper, p.n_rows = 5, 4, 8, 8, 0, 2
    p.lw_dq = (ctypes.c_double * 8)(1.0)
    p.rw, p.huber_delta = 0.0, 0.0
    for k, v in over.items():
        setattr(p, k, v)
    return p


def frame(**over):
    f = _lib.Frame()
    f.views, f.n_views, f.depth_dtype, f.H, f.W = PTR, 2, _lib.F32, 240, 320
    f.K = f.Kinv = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    f.scale, f.half, f.max_dist = 0.025, 32.0, 2.0
    for k, v in over.items():
        setattr(f, k, v)
    return f


def gate(normals=PTR, min_cos=0.5):
    return _lib.NormalGate(normals, min_cos)


def params(**over):
    sp = _lib.SolveParams()
    sp.pcg_iters, sp.lm_abs, sp.lm_rel, sp.step = 10, 0.0, 0.0, 1.0
    sp.x_out, sp.pcg_workspace, sp.pcg_workspace_bytes = PTR, PTR, BIG
    sp.n_iters, sp.n_global, sp.global_lm = 1, 0, 0.1
    sp.global_scratch, sp.global_scratch_bytes = PTR, BIG
    for k, v in over.items():
        setattr(sp, k, v)
    return sp


CALLS = {
    "dfh_gn_associate_gated": lambda lib, p, f, g, **kw: lib.dfh_gn_associate_gated(p, f, g, None),
    "dfh_gn_build_gated": lambda lib, p, f, g, **kw: lib.dfh_gn_build_gated(p, f, g, None),
    "dfh_gn_solve_gated": lambda lib, p, f, g, sp=None, **kw: lib.dfh_gn_solve_gated(p, f, g, params() if sp is None else sp, None),
    "dfh_gn_global_sampled_gated": lambda lib, p, f, g, sp=None, stride=1, n_steps=1, sums=0, scratch=PTR, nbytes=BIG, **kw:
        lib.dfh_gn_global_sampled_gated(p, f, g, stride, 0.1, n_steps, PTR, sums, scratch, nbytes, None),
}
FUSED = ("dfh_gn_build_gated", "dfh_gn_solve_gated")

# what all four refuse: (problem, frame, gate)
BAD = {
    "null problem": lambda: (None, frame(), gate()),
    "null frame": lambda: (problem(), None, gate()),
    "null gate": lambda: (problem(), frame(), None),
    "null normals": lambda: (problem(), frame(), gate(normals=0)),
    "min_cos nan": lambda: (problem(), frame(), gate(min_cos=NAN)),
    "min_cos -0.1": lambda: (problem(), frame(), gate(min_cos=-0.1)),
    "min_cos 1.5": lambda: (problem(), frame(), gate(min_cos=1.5)),
    "min_cos inf": lambda: (problem(), frame(), gate(min_cos=INF)),
    "null views": lambda: (problem(), frame(views=0), gate()),
    "0 views": lambda: (problem(), frame(n_views=0), gate()),
    "17 views": lambda: (problem(), frame(n_views=17), gate()),
    "depth_dtype 2": lambda: (problem(), frame(depth_dtype=2), gate()),
    "H 1": lambda: (problem(), frame(H=1), gate()),
    "scale 0": lambda: (problem(), frame(scale=0.0), gate()),
    "knn 9": lambda: (problem(knn=9), frame(), gate()),
    "null node_dq": lambda: (problem(node_dq=0), frame(), gate()),
    "null sample_nrm": lambda: (problem(sample_nrm=0), frame(), gate()),
    "negative n_samples": lambda: (problem(n_samples=-1), frame(), gate()),
}


def _refused(lib, name, rc, case):
    assert rc == BADARG, (name, case, rc)
    assert name.encode() in lib.dfh_last_error(), (name, case, lib.dfh_last_error())


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("name", sorted(CALLS))
@on_own_thread
def test_bad_problems_frames_and_gates_are_refused(lib, name, case):
    p, f, g = BAD[case]()
    _refused(lib, name, CALLS[name](lib, p, f, g), case)


@pytest.mark.parametrize("name", sorted(CALLS))
@on_own_thread
def test_the_limits_of_min_cos_pass_and_no_samples_launch_nothing(lib, name):
    # (a launch on a machine without a GPU would come back as an error: DFH_OK means that there was none)
    for cos in (0.0, 1.0, 0.5):
        assert CALLS[name](lib, problem(n_samples=0), frame(), gate(min_cos=cos)) == OK, (name, cos)
    # ... but the arguments are checked first
    _refused(lib, name, CALLS[name](lib, problem(n_samples=0), frame(), gate(min_cos=NAN)), "no samples, min_cos nan")
    _refused(lib, name, CALLS[name](lib, problem(n_samples=0), frame(), None), "no samples, null gate")


@pytest.mark.parametrize("name", FUSED)
@on_own_thread
def test_fused_gated_calls_need_a_plan_and_float32_maps(lib, name):
    _refused(lib, name, CALLS[name](lib, problem(), frame(depth_dtype=_lib.F64), gate()), "float64 maps")
    _refused(lib, name, CALLS[name](lib, problem(blk_ptr=0), frame(), gate()), "no plan")
    _refused(lib, name, CALLS[name](lib, problem(vals=0), frame(), gate()), "no system")


@on_own_thread
def test_solve_gated_refuses_bad_schedules(lib):
    name = "dfh_gn_solve_gated"
    assert lib.dfh_gn_solve_gated(problem(), frame(), gate(), None, None) == BADARG
    assert name.encode() in lib.dfh_last_error()
    for case, sp in (("n_iters 1001", params(n_iters=1001)), ("n_iters -1", params(n_iters=-1)), ("n_global 101", params(n_global=101)),
                     ("n_global -1", params(n_global=-1)), ("pcg_iters 0", params(pcg_iters=0)), ("null x_out", params(x_out=0)),
                     ("null workspace", params(pcg_workspace=0))):
        _refused(lib, name, CALLS[name](lib, problem(), frame(), gate(), sp=sp), case)
        _refused(lib, name, CALLS[name](lib, problem(n_samples=0), frame(), gate(), sp=sp), case + ", no samples")


@on_own_thread
def test_sampled_gated_step_refuses_bad_schedules(lib):
    name = "dfh_gn_global_sampled_gated"
    call = CALLS[name]
    _refused(lib, name, call(lib, problem(), frame(), gate(), stride=0), "stride 0")
    _refused(lib, name, call(lib, problem(), frame(), gate(), n_steps=101), "n_steps 101")
    _refused(lib, name, call(lib, problem(), frame(), gate(), n_steps=-1), "n_steps -1")
    need = lib.dfh_gn_global_sampled_bytes(5, 1)
    _refused(lib, name, call(lib, problem(), frame(), gate(), nbytes=need - 1), "scratch too small")
    _refused(lib, name, call(lib, problem(), frame(), gate(), scratch=0), "null scratch")
    _refused(lib, name, call(lib, problem(), frame(), gate(), sums=PTR, n_steps=2), "sums_out with two steps")
    # no step: nothing to check, nothing to launch -- also with a gate that would be refused
    assert call(lib, problem(), frame(), gate(), n_steps=0) == OK
    assert call(lib, problem(), frame(), gate(min_cos=NAN), n_steps=0) == OK
    _refused(lib, name, call(lib, problem(), frame(), gate(), n_steps=0, stride=0), "stride 0 without steps")


def test_the_abi_version_did_not_move_and_the_struct_is_registered(lib):
    assert lib.dfh_version() == 8 == _lib.ABI_VERSION
    for name in CALLS:
        assert name in _lib._SIGNATURES and name in _lib.declared_symbols()
    assert _lib.STRUCTS["dfh_gn_normal_gate"] is _lib.NormalGate
    assert ctypes.sizeof(_lib.NormalGate) == 16
