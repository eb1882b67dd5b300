"""GPU: the normal-compatibility gate of the depth data term (dfh_gn_associate_gated, dfh_gn_build_gated, dfh_gn_solve_gated,
dfh_gn_global_sampled_gated and the Python layers above them) against its numpy restatement (tests/assoc_normals_np.py), against
the ungated calls where the gate cannot bite, and sequence against sequence, bit for bit.  Samples only, no volumes -- except the
frame loop's test at 64^3."""
import functools

import numpy as np
import pytest
import torch

import assoc_normals_np as AN
import assoc_normals_scenes as SC
import depth_prep_cases as C
from dynamicfusion_body_amd import _lib, scene, solve
from dynamicfusion_body_amd.depth_prep import DepthPrep
from dynamicfusion_body_amd.pipeline import SlabFrame
from oracle import gn_np as G

pytestmark = pytest.mark.gpu

MIN_COS = 0.5
TILE = 128
ORBIT5 = (0, 72, 144, 216, 288)                    # five views: one full group of four plus a remainder, and the view cull is on
ANGLES = {"thin": {1: (0,), 2: (0, 180), 5: ORBIT5}, "ordinary": {1: (0,), 2: (-40, 40), 5: ORBIT5}}
MAX_DIST = {"thin": {1: 4.5, 2: 3.0, 5: 3.0}, "ordinary": {1: 2.0, 2: 2.0, 5: 2.0}}
LW = G.twist_exp_dq(np.array([0.004, -0.006, 0.005, 0.2, -0.15, 0.1]))


@pytest.fixture(autouse=True)
def _options_back():
    yield
    _lib.reset_options()


@functools.lru_cache(maxsize=None)
def scene_of(kind, n_views, dtype="float64", n_nodes=32, knn=4, moved=True):
    make = SC.thin if kind == "thin" else SC.ordinary
    move = ((0.0, 0.0, 1.5) if kind == "thin" else (0.6, -0.4, 0.3)) if moved else (0.0, 0.0, 0.0)
    return make(ANGLES[kind][n_views], move=move, n_nodes=n_nodes, knn=knn, depth_dtype=np.dtype(dtype).type)


def field(n_nodes, seed=3):
    """A non-identity warp field: small random twists."""
    rng = np.random.default_rng(seed)
    return np.array([G.twist_exp_dq(rng.normal(size=6) * np.array([.02, .02, .02, .3, .3, .3])) for _ in range(n_nodes)])


class Rig:
    """A WarpSolver on a scene's samples (sorted by node tuple: the device's order is the order of everything below) and the
    scene's maps on the device."""

    def __init__(self, sc, knn, ndq=None, reg=False, nmaps=None):
        self.sc, self.knn = sc, knn
        self.ndq = sc.dqs if ndq is None else ndq
        sv = self.sv = solve.WarpSolver(knn=knn, distributed=False)
        node_nbr = solve.sample_knn(sc.node_pos, sc.node_pos, sc.node_w, knn)[0] if reg else None
        sv.set_graph(sc.node_pos, self.ndq, sc.node_w, node_nbr)
        sv.set_samples(sc.pos, sc.nrm)
        self.pos, self.nrm = sv.spos.cpu().numpy(), sv.snrm.cpu().numpy()
        self.nbr = sv.snbr.cpu().numpy().astype(np.int64)
        self.depth = [torch.from_numpy(d).cuda() for d in sc.dms]
        self.nmaps = sc.nmaps if nmaps is None else nmaps
        self.normals = torch.from_numpy(np.ascontiguousarray(self.nmaps)).cuda()
        self.geom = (SC.K, SC.KINV, sc.lws, SC.SCALE, SC.CENTER, SC.HALF)

    def depth_arg(self):
        return (self.depth, self.sc.lws) if len(self.depth) > 1 else (self.depth[0], self.sc.lws[0])

    def associate(self, lw, max_dist, gated=True, min_cos=MIN_COS, normals=None):
        d, lws = self.depth_arg()
        self.sv.corr.fill_(7.0)
        self.sv.valid.fill_(3)
        kw = {"normals": self.normals if normals is None else normals, "normal_cos": min_cos} if gated else {}
        self.sv.associate_depth(d, SC.K, SC.KINV, lws, SC.SCALE, SC.CENTER, SC.HALF, lw, max_dist, **kw)
        return self.sv.corr.clone(), self.sv.valid.clone()

    def restate(self, lw, max_dist, min_cos=MIN_COS, dqs=None, nmaps=None):
        dqs = self.ndq if dqs is None else dqs
        xw, nw = AN.warped(self.pos, self.nrm, dqs, self.nbr, self.sc.node_pos, self.sc.node_w, lw)
        return AN.associate_depth_views_gated(xw, nw, SC.K, SC.KINV, self.sc.lws, self.sc.dms, self.nmaps if nmaps is None else nmaps,
                                              SC.SCALE, SC.CENTER, SC.HALF, max_dist, min_cos)


def compare(tag, corr, valid, restated, S):
    co, vo, _, edge = restated
    corr, valid = corr.cpu().numpy(), valid.cpu().numpy()
    sure = ~edge
    both = valid.astype(bool) & vo & sure
    err = np.abs(corr[both] - co[both]).max() if both.any() else 0.0
    print("%s: valid %d (restated %d), left out %d, max |corr - restated| %.3g" % (tag, int(valid.sum()), int(vo.sum()), int(edge.sum()), err))
    assert edge.sum() <= 0.001 * S
    assert set(np.unique(valid).tolist()) <= {0, 1}
    assert np.array_equal(valid[sure].astype(bool), vo[sure])
    assert err <= 1e-9
    assert np.all(corr[valid == 0] == 0.0)
    return vo


# ------------------------------------------------------------------------------- the stand-alone kernel
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n_views", [1, 2, 5])
@pytest.mark.parametrize("knn", [1, 3, 4, 8])
@pytest.mark.parametrize("kind", ["thin", "ordinary"])
def test_gated_association_vs_restatement(kind, knn, n_views, dtype):
    sc = scene_of(kind, n_views, dtype)
    rig = Rig(sc, knn, ndq=field(len(sc.node_pos)))
    max_dist = MAX_DIST[kind][n_views]
    corr, valid = rig.associate(LW, max_dist)
    vo = compare("%s knn %d views %d %s" % (kind, knn, n_views, dtype), corr, valid, rig.restate(LW, max_dist), SC.N_SAMPLES)
    # the gate bites: the ungated call keeps more, and everything the gate keeps
    cu, vu = rig.associate(LW, max_dist, gated=False)
    vu = vu.cpu().numpy().astype(bool)
    assert 0 < vo.sum() < vu.sum() and not (vo & ~vu).any()
    # ragged last tile, and (one view: the far side of the ball) tiles without a valid sample
    per_tile = np.add.reduceat(vo.astype(np.int64), np.arange(0, SC.N_SAMPLES, TILE))
    assert SC.N_SAMPLES % TILE != 0 and (n_views > 1 or (per_tile == 0).sum() >= 5)


def test_a_rejected_nearer_view_lets_a_farther_compatible_one_win():
    """Two opposite views of the thin ball: without the gate the nearest surface wins whichever side it is; with it some samples keep
    ANOTHER view's correspondence than the ungated call chose -- the gate sits in front of the comparison."""
    rig = Rig(scene_of("thin", 2), 4)
    xw, nw = AN.warped(rig.pos, rig.nrm, rig.ndq, rig.nbr, rig.sc.node_pos, rig.sc.node_w, SC.IDENT)
    _, vu, view_u = G.associate_depth_views(xw, SC.K, SC.KINV, rig.sc.lws, rig.sc.dms, SC.SCALE, SC.CENTER, SC.HALF, 3.0)
    co, vo, view_g, edge = rig.restate(SC.IDENT, 3.0)
    switched = vo & vu & (view_g != view_u)
    assert switched.sum() > 10 and not edge.any()
    corr, valid = rig.associate(SC.IDENT, 3.0)
    assert np.abs(corr.cpu().numpy()[switched] - co[switched]).max() <= 1e-9 and valid.cpu().numpy()[switched].all()


# ------------------------------------------------------------------------------- anchor to the ungated path
@pytest.mark.parametrize("kind,n_views", [("ordinary", 5), ("thin", 2), ("ordinary", 1)])
def test_a_gate_that_cannot_bite_is_the_ungated_association(kind, n_views):
    """Every sample carries the same normal n0 under the identity field and every pixel of view v holds R_v n0: the cosine is 1 up
    to float32 rounding of the map (1 - O(1e-14)), so any min_cos <= 1 - 1e-6 passes every correspondence."""
    sc = scene_of(kind, n_views, "float32")
    n0 = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    nmaps = np.stack([np.broadcast_to((lw[:, :3] @ n0).astype(np.float32), (SC.H, SC.W, 3)) for lw in sc.lws])
    rig = Rig(sc, 4, nmaps=nmaps)
    rig.sv.snrm.copy_(torch.from_numpy(np.tile(n0, (SC.N_SAMPLES, 1))))
    cu, vu = rig.associate(SC.IDENT, MAX_DIST[kind][n_views], gated=False)
    assert vu.sum() > 100
    for cos in (0.0, 0.5, 1.0 - 1e-6):
        cg, vg = rig.associate(SC.IDENT, MAX_DIST[kind][n_views], min_cos=cos)
        assert torch.equal(cg, cu) and torch.equal(vg, vu), cos
    # ... and the opposite normal passes nothing
    rig.sv.snrm.copy_(torch.from_numpy(np.tile(-n0, (SC.N_SAMPLES, 1))))
    cg, vg = rig.associate(SC.IDENT, MAX_DIST[kind][n_views], min_cos=0.0)
    assert vg.sum() == 0 and bool((cg == 0).all())


# ------------------------------------------------------------------------------- bad normal values
def test_bad_normal_values():
    """NaN, +-inf, zero and length-2 normals at pixels that samples land on: the device decides as the restatement does (a NaN
    fails, a pixel without a normal fails), and the test is scale-free."""
    sc = scene_of("ordinary", 2, "float32")
    rig = Rig(sc, 4)
    xw, _ = AN.warped(rig.pos, rig.nrm, rig.ndq, rig.nbr, sc.node_pos, sc.node_w, SC.IDENT)
    _, v0, _, _ = rig.restate(SC.IDENT, 2.0)
    nmaps = sc.nmaps.copy()
    planted = {}
    for view in range(2):
        ui, vi, inside = AN.pixels(xw, SC.K, sc.lws[view], SC.H, SC.W, SC.SCALE, SC.CENTER, SC.HALF)
        land = np.unique(np.stack([vi, ui], axis=1)[inside & v0], axis=0)
        assert len(land) > 200
        for j, (name, make) in enumerate((("nan", lambda n: np.array([np.nan, n[1], n[2]])), ("+inf", lambda n: np.array([n[0], np.inf, n[2]])),
                                          ("-inf", lambda n: np.array([n[0], n[1], -np.inf])), ("zero", lambda n: np.zeros(3)),
                                          ("all nan", lambda n: np.full(3, np.nan)), ("length 2", lambda n: 2.0 * n))):
            for y, x in land[j::12][:15]:
                nmaps[view, y, x] = make(nmaps[view, y, x]).astype(np.float32)
                planted[name] = planted.get(name, 0) + 1
    assert min(planted.values()) >= 10, planted
    normals = torch.from_numpy(nmaps).cuda()
    with np.errstate(all="ignore"):
        restated = rig.restate(SC.IDENT, 2.0, nmaps=nmaps)
    corr, valid = rig.associate(SC.IDENT, 2.0, normals=normals)
    vo = compare("bad normals", corr, valid, restated, SC.N_SAMPLES)
    assert vo.sum() < v0.sum()                                     # (the planted values cost correspondences)
    assert bool(torch.isfinite(corr).all())
    # scale-free: every normal doubled (exact in float32) decides the same and leaves the same bits
    c2, v2 = rig.associate(SC.IDENT, 2.0, normals=normals * 2.0)
    assert torch.equal(c2, corr) and torch.equal(v2, valid)


# ------------------------------------------------------------------------------- the fused build
def system(sv):
    return sv.corr.clone(), sv.valid.clone(), sv.vals.clone(), sv.rhs.clone(), sv.cost_count.clone()


@pytest.mark.parametrize("cull", [True, False])
@pytest.mark.parametrize("kind,n_views,knn,dead,full", [("ordinary", 5, 3, True, True), ("ordinary", 5, 1, True, True), ("ordinary", 2, 4, True, True),
                                                        ("thin", 5, 1, True, False), ("ordinary", 5, 8, False, True)])
def test_fused_gated_build_is_associate_then_build(kind, n_views, knn, dead, full, cull):
    """Five views: the per-tile view cull is on (and, with gn_no_view_cull, off); two views: it never is.  dead / full: the case has
    tiles without a valid sample / with 128 of them; the last tile of every case is ragged."""
    sc = scene_of(kind, n_views, "float32")
    rig = Rig(sc, knn, ndq=field(len(sc.node_pos)), reg=True)
    sv = rig.sv
    d, lws = rig.depth_arg()
    args = (d, SC.K, SC.KINV, lws, SC.SCALE, SC.CENTER, SC.HALF, LW, 5.0, MAX_DIST[kind][n_views], 0.5)
    if not cull:
        _lib.set_option("gn_no_view_cull", 1)
    sv.build_associated(*args, normals=rig.normals, normal_cos=MIN_COS)
    fused = system(sv)
    _lib.set_option("py_gn_no_fused_assoc", 1)
    sv.corr.fill_(7.0); sv.valid.fill_(3); sv.vals.fill_(7.0); sv.rhs.fill_(7.0)
    sv.build_associated(*args, normals=rig.normals, normal_cos=MIN_COS)
    two = system(sv)
    for name, a, b in zip(("corr", "valid", "vals", "rhs", "cost_count"), fused, two):
        assert torch.equal(a, b), name
    v = fused[1].cpu().numpy().astype(np.int64)
    per_tile = np.add.reduceat(v, np.arange(0, SC.N_SAMPLES, TILE))
    assert int(fused[4][1]) == v.sum() > 100
    assert bool((per_tile == 0).any()) == dead and bool((per_tile == TILE).any()) == full, per_tile.tolist()
    # ... and it is the gated association: not the ungated build's system
    _lib.set_option("py_gn_no_fused_assoc", None)
    sv.build_associated(*args)
    assert not torch.equal(sv.valid, fused[1]) and int(sv.cost_count[1]) > v.sum()


def test_the_atomic_build_takes_the_gated_association_too():
    sc = scene_of("ordinary", 2, "float32")
    rig = Rig(sc, 4, ndq=field(len(sc.node_pos)), reg=True)
    sv = rig.sv
    d, lws = rig.depth_arg()
    args = (d, SC.K, SC.KINV, lws, SC.SCALE, SC.CENTER, SC.HALF, LW, 5.0, 2.0, 0.0)
    sv.build_associated(*args, normals=rig.normals, normal_cos=MIN_COS)
    planned = system(sv)
    _lib.set_option("py_gn_atomic", 1)
    sv.build_associated(*args, normals=rig.normals, normal_cos=MIN_COS)
    atomic = system(sv)
    assert torch.equal(planned[0], atomic[0]) and torch.equal(planned[1], atomic[1])
    for a, b in zip(planned[2:], atomic[2:]):                       # (atomics: another summation order)
        assert float((a - b).abs().max()) <= 1e-9 * max(1.0, float(a.abs().max()))


# ------------------------------------------------------------------------------- the one-call solve
SEQUENCES = {"one call": (), "per-iteration calls": ("py_gn_iter_per_call",), "build and solve calls": ("py_gn_no_fused_iter",),
             "associate, build and solve calls": ("py_gn_no_fused_assoc",)}


@pytest.mark.parametrize("kind,n_views", [("ordinary", 5), ("thin", 2)])
def test_every_gated_solve_sequence_leaves_the_same_bits(kind, n_views):
    sc = scene_of(kind, n_views, "float32")
    start = field(len(sc.node_pos))
    rig = Rig(sc, 4, ndq=start, reg=True)
    sv = rig.sv
    d, lws = rig.depth_arg()
    start_t = sv.node_dq.clone()
    out = {}
    for name, options in SEQUENCES.items():
        for o in options:
            _lib.set_option(o, 1)
        sv.node_dq.copy_(start_t)
        sv.iterate_associated(d, SC.K, SC.KINV, lws, SC.SCALE, SC.CENTER, SC.HALF, LW, 5.0, MAX_DIST[kind][n_views], 0.5, 10.0, 1e-2,
                              n_iters=3, n_global=1, global_lm=0.1, normals=rig.normals, normal_cos=MIN_COS)
        torch.cuda.synchronize()
        sv.check_status()
        out[name] = (sv.node_dq.clone(), sv.valid.clone(), sv.corr.clone(), sv.cost_count.clone())
        _lib.reset_options()
    ref = out["one call"]
    assert not torch.equal(ref[0], start_t) and bool(torch.isfinite(ref[0]).all())
    for name, got in out.items():
        for a, b in zip(ref, got):
            assert torch.equal(a, b), name
    # the gate steered it: the ungated schedule ends elsewhere
    sv.node_dq.copy_(start_t)
    sv.iterate_associated(d, SC.K, SC.KINV, lws, SC.SCALE, SC.CENTER, SC.HALF, LW, 5.0, MAX_DIST[kind][n_views], 0.5, 10.0, 1e-2,
                          n_iters=3, n_global=1, global_lm=0.1)
    assert not torch.equal(sv.node_dq, ref[0])


# ------------------------------------------------------------------------------- the sampled rigid-mode step
@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("kind,n_views,knn", [("thin", 1, 4), ("ordinary", 5, 8), ("thin", 2, 1)])
def test_sampled_gated_step_vs_oracle(kind, n_views, knn, dtype, stride):
    sc = scene_of(kind, n_views, dtype)
    start = field(len(sc.node_pos))
    rig = Rig(sc, knn, ndq=start)
    sv = rig.sv
    d, lws = rig.depth_arg()
    max_dist, huber = MAX_DIST[kind][n_views], 0.5
    sv.global_sampled(d, SC.K, SC.KINV, lws, SC.SCALE, SC.CENTER, SC.HALF, LW, max_dist, huber, 0.1, n_steps=1, stride=stride,
                      normals=rig.normals, normal_cos=MIN_COS)
    xi = sv.global_xi.cpu().numpy()
    edges = []

    def associate(xw):
        _, nw = AN.warped(rig.pos, rig.nrm, start, rig.nbr, sc.node_pos, sc.node_w, LW)
        c, v, _, e = AN.associate_depth_views_gated(xw, nw, SC.K, SC.KINV, sc.lws, sc.dms, sc.nmaps, SC.SCALE, SC.CENTER, SC.HALF, max_dist, MIN_COS)
        edges.append(int(e.sum()))
        return c, v
    dqs, xi_o, count = G.global_step_sampled(start, rig.pos, rig.nrm, rig.nbr, sc.node_pos, sc.node_w, LW, associate, huber, 0.1, stride=stride)
    print("%s views %d knn %d %s stride %d: valid %d (oracle %d), max |xi - oracle| %.3g, max |dq - oracle| %.3g" % (
        kind, n_views, knn, dtype, stride, int(xi[7]), count, np.abs(xi[:6] - xi_o).max(), np.abs(sv.node_dq.cpu().numpy() - dqs).max()))
    assert edges == [0]
    assert int(xi[7]) == count > 6
    assert np.abs(xi[:6] - xi_o).max() <= 1e-9
    assert np.abs(sv.node_dq.cpu().numpy() - dqs).max() <= 1e-9


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_the_gated_rigid_step_recovers_the_thin_balls_motion(dtype):
    """tests/test_assoc_normals_cpu.py's displacement assertions for the device's DQs: one view of the thin ball moved by 1.5 voxels
    along z, 16 nodes, knn 4, lm_rel 0.1, no Huber, one step from the identity."""
    sc = scene_of("thin", 1, dtype, n_nodes=16)
    dz = {}
    for gated in (False, True):
        rig = Rig(sc, 4)
        kw = {"normals": rig.normals, "normal_cos": MIN_COS} if gated else {}
        d, lws = rig.depth_arg()
        rig.sv.global_sampled(d, SC.K, SC.KINV, lws, SC.SCALE, SC.CENTER, SC.HALF, SC.IDENT, 4.5, 0.0, 0.1, n_steps=1, stride=1, **kw)
        dq = rig.sv.node_dq.cpu().numpy()
        assert np.abs(dq - dq[0]).max() == 0.0                      # one twist for all nodes
        dz[gated] = SC.centre_displacement(dq[0])[2]
    print("centre displacement along z (true 1.5): ungated %.4f, gated %.4f" % (dz[False], dz[True]))
    assert dz[True] > 1.0 and dz[False] < 0.5


# ------------------------------------------------------------------------------- the Python layer's refusals
def test_bad_normal_maps_are_refused_before_any_launch():
    rig = Rig(scene_of("thin", 2, "float32"), 4)
    for bad in (rig.normals[:1], rig.normals.double(), rig.normals[:, :, :, :2], rig.normals.cpu(), rig.normals.permute(0, 2, 1, 3)):
        with pytest.raises(ValueError):
            rig.associate(SC.IDENT, 3.0, normals=bad)
    for cos in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            rig.associate(SC.IDENT, 3.0, min_cos=cos)


# ------------------------------------------------------------------------------- the frame loop
R, N = 64, 64
FH, FW = 37, 53
FRAME_ANGLES = (0.0, 40.0)


def prep():
    return DepthPrep(radius=2, sigma_s=1.5, sigma_r=0.05, max_jump=C.SCENE_JUMP, min_cos=0.5)


@pytest.fixture(scope="module")
def frames():
    K = C.small_camera()
    scale = scene.grid_params(R)[0]
    lws = [scene.view_extrinsic(a) for a in FRAME_ANGLES]
    out = []
    for f in range(2):                                                         # frame 0 builds the canonical volume
        off = np.array([0.4, -0.25, 0.15]) * np.sin(0.5 * f) * scale
        out.append([torch.from_numpy(scene.render_depth(K, lw, FH, FW, dtype=np.float32, invalid_frac=0.02, seed=11 + f,
                                                        sphere_offset=off)).cuda() for lw in lws])
    return K, lws, out


def new_loop(K, lws, first, **kw):
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    sf = SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, knn=4, pcg_iters=10, band=2.0, distributed=False, **kw)
    for d, lw in zip(first, lws):
        sf.integrate(d, lw)
    assert sf.refresh_samples() > 100
    return sf


def state(sf):
    torch.cuda.synchronize()
    return sf.T.clone(), sf.Wt.clone(), sf.fs.solver.node_dq.clone()


def test_slab_frame_steps_through_the_gate(frames):
    K, lws, fr = frames
    gated, keyword, plain = (new_loop(K, lws, fr[0], depth_prep=prep(), normal_gate=0.5), new_loop(K, lws, fr[0], depth_prep=prep()),
                             new_loop(K, lws, fr[0], depth_prep=prep()))
    counts = {}
    for name, sf, kw in (("gated", gated, {}), ("keyword", keyword, {"normal_gate": 0.5}), ("plain", plain, {})):
        assert sf.step(fr[1], lws, gn_iters=3, global_stride=1, **kw) > 100
        counts[name] = int(sf.fs.solver.global_xi[7])                          # valid samples of the last rigid-mode step (every tile)
    print("valid samples in the rigid-mode step:", counts)
    assert 6 < counts["gated"] == counts["keyword"] < counts["plain"]
    sg, sk, sp = state(gated), state(keyword), state(plain)
    assert all(torch.equal(a, b) for a, b in zip(sg, sk))                      # the constructor's value and the keyword: one path
    assert not all(torch.equal(a, b) for a, b in zip(sg, sp))
    assert all(bool(torch.isfinite(t).all()) for t in sg)


def test_no_gate_leaves_the_bits_of_a_step_that_never_heard_of_it(frames):
    K, lws, fr = frames
    a, b, c = (new_loop(K, lws, fr[0], depth_prep=prep()), new_loop(K, lws, fr[0], depth_prep=prep()),
               new_loop(K, lws, fr[0], depth_prep=prep(), normal_gate=0.5))
    a.step(fr[1], lws, gn_iters=3)
    b.step(fr[1], lws, gn_iters=3, normal_gate=None)
    c.step(fr[1], lws, gn_iters=3, normal_gate=None)                           # (the keyword overrides the constructor's value)
    sa = state(a)
    assert all(torch.equal(x, y) for x, y in zip(sa, state(b))) and all(torch.equal(x, y) for x, y in zip(sa, state(c)))


def test_the_gate_needs_normal_maps_and_the_depth_term(frames):
    K, lws, fr = frames
    scale, center, tdist = scene.grid_params(R)
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    with pytest.raises(ValueError, match="depth_prep"):
        SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, distributed=False, normal_gate=0.5)
    with pytest.raises(ValueError, match="normal_gate"):
        SlabFrame(K, scale, center, R, tdist / scale, node_pos, node_w, distributed=False, depth_prep=prep(), normal_gate=1.5)
    sf = new_loop(K, lws, fr[0])
    before = state(sf)
    with pytest.raises(ValueError, match="depth_prep"):
        sf.step(fr[1], lws, gn_iters=1, normal_gate=0.5)
    with_prep = new_loop(K, lws, fr[0], depth_prep=prep())
    with pytest.raises(ValueError, match="data_term"):
        with_prep.step(fr[1], lws, gn_iters=1, normal_gate=0.5, data_term="volume")
    assert all(torch.equal(x, y) for x, y in zip(before, state(sf)))           # refused before anything ran
