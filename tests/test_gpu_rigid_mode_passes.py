"""GPU: the rigid-mode rows kernel (gn_global_rows_kernel, csrc/dfh_gn_global.hip) past the first pass of its grid.

The kernel runs at most GRID = 1536 workgroups; workgroup b walks the thinned 128-sample tiles b, b + 1536, ... and keeps ONE
matrix-core accumulator (and its objective and count) across them, rewriting the same LDS rows for every tile behind a wave
barrier.  The other tests of the step (tests/test_gpu_configs.py, test_gpu_volume_fused.py, test_gpu_assoc_normals.py) stay below
a few hundred tiles: no workgroup there takes a second one.  Here every association mode -- the views (dfh_gn_global_sampled),
the live volume (dfh_gn_global_sampled_volume), the views through the normal gate (dfh_gn_global_sampled_gated) -- runs on the
scene of its own test file with the samples multiplied until S = 2047 * 128 + 1, so that stride 1 has 2048 thinned tiles: a second
pass for the first 512 workgroups, and a last tile of ONE sample.  (512, not one or two: the samples are sorted by node tuple, and
the first tiles of the views' scene hold no valid row at all -- a workgroup that lost its first tile there would lose nothing.)
The views' and the gate's scenes are replicated, each replica moved by its own sub-voxel offset (no two passes hold the same
rows); the volume's ray samples are simply drawn in that number.

Cases per mode: stride 1 (two passes) and stride 3 (683 tiles: one pass, the control) at S = 2047 * 128 + 1; stride 1 at
S = 1536 * 128 (exactly the grid) and at S = 1537 * 128 - 5 (1537 tiles: the second pass is one tile of 123 samples).  The oracle is
oracle/gn_np.global_step_sampled on the DEVICE's sample order, at the bars of those files: valid count exact, twist to 1e-9
relative, node DQs to 1e-9.  The 29 sums (sums_out, the sharded form of the step) go against J_g^T J_g, J_g^T r and the Huber
objective of the same rows (28 sums), the count exactly.

The bar of the sums.  Measured |device - oracle| / sum |term|, worst of the 28 entries, on each mode's ORIGINAL single-pass
sample set (SINGLE below: S samples, figure), is allowed to grow with the number of additions: a case is held to that figure
times (samples of its thinned tiles) / S_single -- at stride 3 a third of S.  SINGLE holds the measured figures; every run measures
the single-pass set again and holds it to its record, so that a drift of the record shows.

gn_global_step_kernel, the step from the BUILT system, strides 64 x 4 waves over the nodes' right-hand sides: the last test runs
it at 320 nodes, where the first 64 waves take a second node (every other test of that step has at most 216).

Sensitivity, on the CPU inside the same test: with the tiles of the second pass (sub >= 1536) taken out of the oracle's selection
its twist moves by more than 100 times the 1e-9 bar -- the bar can see a dropped pass; and at S = 2047 * 128 + 1 likewise with the
FIRST tiles of the workgroups that take two (sub < 512) taken out -- the bar can see an accumulator that forgot them."""
import numpy as np
import pytest
import torch

import assoc_normals_np as AN
import assoc_normals_scenes as SC
from oracle import gn_np as G
from oracle import oracle_np as O
from dynamicfusion_body_amd import _lib, scene, solve
from dynamicfusion_body_amd.device import current_stream_ptr
from dynamicfusion_body_amd.pipeline import FrameSolver
from test_gpu_associate_volume import ray_samples, restate, sphere_scene
from test_gpu_assoc_normals import LW as GATE_LW, MIN_COS, field, scene_of
from test_gpu_configs import IDENT, _rigid_scene

pytestmark = pytest.mark.gpu

TILE, GRID = 128, 1536
EXTRA = 512                                        # workgroups that take a second tile at S_MULTI, stride 1
S_MULTI = (GRID + EXTRA - 1) * TILE + 1            # 2048 tiles: two passes, the last tile one sample
HUBER, LM_REL = 0.5, 0.1
PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]

S_1537 = (GRID + 1) * TILE - 5                     # 1537 tiles: the second pass is one tile of 123 samples
# (S, stride): thinned tiles, passes
CASES = {(S_MULTI, 1): (GRID + EXTRA, 2), (S_MULTI, 3): (683, 1), (GRID * TILE, 1): (GRID, 1), (S_1537, 1): (GRID + 1, 2)}

# (mode, knn): (S of the single-pass set, worst |device - oracle| / sum |term| of its 28 sums), measured on an MI355X
# (2.47e-14, 3.12e-15, 7.72e-15 and 2.27e-14, rounded up; at S = 262 017 and stride 1 the same runs gave 2.2e-14, 9.6e-15, 2.7e-14 and
# 5.2e-14 against bars of 7.0e-13, 2.1e-13, 5.2e-13 and 6.4e-13 (a third of that at stride 3: 2.7e-14, 1.2e-14, 1.5e-14): the deviation is the rows' own, it hardly grows with the additions)
SINGLE = {("views", 4): (9416, 2.5e-14), ("volume", 4): (4000, 3.2e-15), ("gated", 4): (4000, 7.8e-15), ("views", 8): (9416, 2.3e-14)}


def n_sub(S, stride):
    return -(-(-(-S // TILE)) // stride)


def replicate(pos, nrm, S, seed, amp=0.25):
    """S samples from copies of (pos, nrm), copy j moved by its own offset within +-amp voxels (copy 0 stays)."""
    reps = -(-S // len(pos))
    off = np.random.default_rng(seed).uniform(-amp, amp, size=(reps, 3))
    off[0] = 0.0
    return (pos[None] + off[:, None]).reshape(-1, 3)[:S].copy(), np.tile(nrm, (reps, 1))[:S].copy()


class Mode:
    """One association mode on its scene: a WarpSolver with the graph set, the start field, the device's step and sums, and the
    restated association for the oracle.  single: the scene's own samples; pos_all, nrm_all: the multiplied ones."""

    def set_samples(self, S=None):
        """S = None: the scene's own single-pass set."""
        pos, nrm = self.single if S is None else (self.pos_all[:S], self.nrm_all[:S])
        self.sv.set_samples(pos, nrm)
        assert self.sv.S == len(pos)
        # the device's order is the order of everything below
        self.pos, self.nrm = self.sv.spos.cpu().numpy(), self.sv.snrm.cpu().numpy()
        self.nbr = self.sv.snbr.cpu().numpy().astype(np.int64)
        self._assoc = None

    def reset(self):
        self.sv.node_dq.copy_(torch.from_numpy(self.dq0).cuda())

    def associate(self, xw):
        """(corr, valid) of the warped samples; the oracle and the sums ask for the same points: computed once."""
        if self._assoc is None or not np.array_equal(self._assoc[0], xw):
            self._assoc = (xw, self.restated(xw))
        return self._assoc[1]

    def sums(self, stride):
        """The sharded form: one step's 29 sums, nothing applied."""
        sv = self.sv
        out = torch.full((32,), np.nan, dtype=torch.float64, device="cuda")
        call, against, name = self.entry()
        _lib.check(call(sv._problem(self.lw, huber=HUBER), against, int(stride), LM_REL, 1, 0, out.data_ptr(), sv._gs_ws.data_ptr(),
                        sv._gs_ws.numel() * 8, current_stream_ptr()), name)
        return out.cpu().numpy()[:29]


class Views(Mode):
    name = "views"

    def __init__(self, knn, dtype):
        s = _rigid_scene()
        R, N = s["R"], s["N"]
        fs = FrameSolver(s["K"], s["scale"], s["center"], R / 2, knn=knn, pcg_iters=10, distributed=False)
        fs.set_graph(s["node_pos"], np.tile(IDENT, (N, 1)), s["node_w"])
        self.S_single = fs.set_canonical(s["T"], s["Wt"], band=2.0)
        assert self.S_single > 5000
        self.sv, self.s, self.lw, self.dq0 = fs.solver, s, IDENT, s["dq0"]
        self.node_pos, self.node_w = s["node_pos"], s["node_w"]
        self.lives = [d.astype(dtype) for d in s["live64"]]
        self.depths = [torch.from_numpy(d).cuda() for d in self.lives]
        self.single = (self.sv.spos.cpu().numpy(), self.sv.snrm.cpu().numpy())
        self.pos_all, self.nrm_all = replicate(*self.single, S_MULTI, 21)
        self.geom = (s["K"], s["Kinv"], s["lws"], s["scale"], s["center"], R / 2)

    def step(self, stride):
        K, Kinv, lws, scale, center, half = self.geom
        self.sv.global_sampled(self.depths, K, Kinv, lws, scale, center, half, self.lw, 2.0, HUBER, LM_REL, n_steps=1, stride=stride)

    def entry(self):
        K, Kinv, lws, scale, center, half = self.geom
        return self.sv.lib.dfh_gn_global_sampled, self.sv._frame(self.depths, lws, K, Kinv, scale, center, half, 2.0), "dfh_gn_global_sampled"

    def restated(self, xw):
        K, Kinv, lws, scale, center, half = self.geom
        return G.associate_depth_views(xw, K, Kinv, lws, self.lives, scale, center, half, 2.0)[:2]


class Volume(Mode):
    name = "volume"

    def __init__(self, knn, dtype):
        sc = self.sc = sphere_scene()
        self.S_single = 4000
        self.single = ray_samples(self.S_single, sc)
        self.pos_all, self.nrm_all = ray_samples(S_MULTI, sc)
        self.sv = solve.WarpSolver(knn=knn, pcg_iters=10, distributed=False)
        self.sv.set_graph(sc["npos"], sc["ndq"], sc["nw"])
        self.lw, self.dq0, self.node_pos, self.node_w = sc["lw"], sc["ndq"], sc["npos"], sc["nw"]
        self.live = sc["live"].astype(dtype)
        self.live_t = torch.from_numpy(self.live).cuda()

    def step(self, stride):
        self.sv.global_sampled_volume(self.live_t, self.lw, 4.0, max_dist=2.0, huber=HUBER, lm_rel=LM_REL, n_steps=1, stride=stride, min_grad=0.5)

    def entry(self):
        return self.sv.lib.dfh_gn_global_sampled_volume, self.sv._volume_term(self.live_t, 4.0, 2.0, 0.5, 1.0), "dfh_gn_global_sampled_volume"

    def restated(self, xw):
        c, v, _, margin, _ = restate(xw, self.live, 1.0, 4.0, 2.0, 0.5)
        self.margin = float(margin.min())
        return c, v


class Gated(Mode):
    name = "gated"

    def __init__(self, knn, dtype):
        sc = self.sc = scene_of("ordinary", 5, np.dtype(dtype).name, 32, knn)
        self.S_single = SC.N_SAMPLES
        self.dq0 = field(len(sc.node_pos))
        self.sv = solve.WarpSolver(knn=knn, distributed=False)
        self.sv.set_graph(sc.node_pos, self.dq0, sc.node_w, None)
        self.lw, self.node_pos, self.node_w = GATE_LW, sc.node_pos, sc.node_w
        self.single = (sc.pos, sc.nrm)
        self.pos_all, self.nrm_all = replicate(sc.pos, sc.nrm, S_MULTI, 22)
        self.depths = [torch.from_numpy(d).cuda() for d in sc.dms]
        self.normals = torch.from_numpy(np.ascontiguousarray(sc.nmaps)).cuda()
        self.geom = (SC.K, SC.KINV, sc.lws, SC.SCALE, SC.CENTER, SC.HALF)
        self.edges = 0

    def step(self, stride):
        self.sv.global_sampled(self.depths, *self.geom, self.lw, 2.0, HUBER, LM_REL, n_steps=1, stride=stride, normals=self.normals,
                               normal_cos=MIN_COS)

    def entry(self):
        sv = self.sv
        frame = sv._frame(self.depths, self.sc.lws, SC.K, SC.KINV, SC.SCALE, SC.CENTER, SC.HALF, 2.0)
        gate = sv._gate(self.normals, MIN_COS, frame)
        return (lambda prob, frm, *rest: sv.lib.dfh_gn_global_sampled_gated(prob, frm, gate, *rest)), frame, "dfh_gn_global_sampled_gated"

    def restated(self, xw):
        _, nw = AN.warped(self.pos, self.nrm, self.dq0, self.nbr, self.node_pos, self.node_w, self.lw)
        c, v, _, e = AN.associate_depth_views_gated(xw, nw, SC.K, SC.KINV, self.sc.lws, self.sc.dms, self.sc.nmaps, SC.SCALE, SC.CENTER, SC.HALF,
                                                    2.0, MIN_COS)
        self.edges = int(e.sum())
        return c, v


MODES = {"views": Views, "volume": Volume, "gated": Gated}


def oracle_rows(m, stride):
    """The oracle's rows of the thinned tiles, Huber-scaled: X (n, 7) = {J_g | r}, the rows' thinned tile index, the objective."""
    warped = O.warp(m.pos, m.dq0[m.nbr], m.node_pos[m.nbr], m.node_w[m.nbr], m_lw=m.lw)
    corr, valid = m.associate(warped)
    tile = np.arange(len(m.pos)) // TILE
    sel = np.flatnonzero(valid & (tile % stride == 0))
    r, J = G.data_residual_jacobian(m.dq0, m.pos[sel], m.nrm[sel], corr[sel], m.nbr[sel], m.node_pos, m.node_w, m.lw)
    sc, obj = G.huber_scale(r, HUBER)
    return np.concatenate([(J * sc[:, None, None]).sum(axis=1), (r * sc)[:, None]], axis=1), tile[sel] // stride, obj


def twist_of(X):
    A = X[:, :6].T @ X[:, :6]
    return -np.linalg.solve(A + LM_REL * np.diag(np.diag(A)), X[:, :6].T @ X[:, 6])


def sums_deviation(m, stride):
    """(worst |device - oracle| / sum |term| of the 28 sums -- A_g, g_g and the objective --, the oracle's rows); the count exactly."""
    got = m.sums(stride)
    X, sub, obj = oracle_rows(m, stride)
    terms = np.stack([X[:, i] * X[:, j] for i, j in PAIRS] + [X[:, i] * X[:, 6] for i in range(6)], axis=1)
    want = np.concatenate([terms.sum(axis=0), [obj]])
    mag = np.concatenate([np.abs(terms).sum(axis=0), [obj]])           # (the objective's terms are positive)
    assert got[28] == len(X), (m.name, stride, got[28], len(X))
    return float((np.abs(got[:28] - want) / mag).max()), X, sub


def run_case(name, knn, dtype, S, stride):
    m = MODES[name](knn, np.dtype(dtype).type)
    # the single-pass set the bar is scaled from: the scene's own samples
    m.set_samples()
    m.reset()
    m.step(1)                                                           # (allocates the step's workspace)
    m.reset()
    assert n_sub(m.S_single, 1) < GRID
    single = sums_deviation(m, 1)[0]
    S_rec, dev_rec = SINGLE[(name, knn)]
    print(name, "knn", knn, np.dtype(dtype).name, "single pass: S", m.S_single, "deviation of the sums", single, "recorded", S_rec, dev_rec)
    assert S_rec == m.S_single and single <= dev_rec
    # the multiplied samples
    tiles, passes = CASES[(S, stride)]
    assert n_sub(S, stride) == tiles and -(-tiles // GRID) == passes
    m.set_samples(S)
    m.reset()
    m.step(stride)
    xi = m.sv.global_xi.cpu().numpy()
    dq = m.sv.node_dq.cpu().numpy()
    dq_o, xi_o, n_o = G.global_step_sampled(m.dq0, m.pos, m.nrm, m.nbr, m.node_pos, m.node_w, m.lw, m.associate, HUBER, LM_REL, stride=stride,
                                            tile=TILE)
    tag = (name, knn, S, stride)
    if name == "volume":
        print("smallest margin of a decision", m.margin)
        assert m.margin > 1e-9                                         # (no decision of the restatement close to flipping)
    if name == "gated":
        assert m.edges == 0
    print(tag, "tiles", tiles, "valid", int(xi[7]), "oracle", n_o, "max |xi - oracle|", float(np.abs(xi[:6] - xi_o).max()),
          "max |dq - oracle|", float(np.abs(dq - dq_o).max()))
    assert int(xi[7]) == n_o and n_o > 0.05 * S / stride, tag
    assert np.abs(xi[:6] - xi_o).max() <= 1e-9 * max(1.0, np.abs(xi_o).max()), (tag, xi[:6], xi_o)
    assert np.abs(dq - dq_o).max() <= 1e-9, tag
    assert np.abs(xi_o).max() > 1e-3, tag                              # (a real step)
    # the 29 sums of the sharded form
    m.reset()
    dev, X, sub = sums_deviation(m, stride)
    assert np.array_equal(m.sv.node_dq.cpu().numpy(), m.dq0)            # (the sums alone apply nothing)
    assert np.abs(twist_of(X) - xi_o).max() <= 1e-12 * max(1.0, np.abs(xi_o).max())       # (the two statements of the oracle agree)
    thinned = int(((np.arange(S) // TILE) % stride == 0).sum())       # the samples whose rows this case adds
    bar = dev_rec * thinned / S_rec
    print(tag, "deviation of the sums", dev, "bar", bar)
    assert dev <= bar, (tag, dev, bar)
    assert sub.max() < tiles and (sub >= GRID).any() == (passes > 1)
    if passes > 1:
        # the bars see a dropped second pass: without the tiles a workgroup reaches only in the second turn of its loop the oracle's
        # twist moves by more than 100 times the 1e-9 bar
        moved = float(np.abs(twist_of(X[sub < GRID]) - xi_o).max())
        print(tag, "rows of the second pass", int((sub >= GRID).sum()), "the twist without them moves by", moved)
        assert moved >= 100 * 1e-9 * max(1.0, np.abs(xi_o).max())
    if tiles == GRID + EXTRA:
        # and an accumulator that forgot the first tile of the workgroups that take two
        first = sub < EXTRA
        moved = float(np.abs(twist_of(X[~first]) - xi_o).max())
        print(tag, "rows of the first tiles of the workgroups that take two", int(first.sum()), "the twist without them moves by", moved)
        assert moved >= 100 * 1e-9 * max(1.0, np.abs(xi_o).max())


@pytest.mark.parametrize("S,stride", list(CASES))
@pytest.mark.parametrize("name", ["views", "volume", "gated"])
def test_rigid_mode_rows_past_the_first_pass(name, S, stride):
    """knn = 4, float32 maps / volume, every association mode, every case.  Measured on an MI355X, deviation of the 28 sums on the
    single-pass set -> at S = 262 017, stride 1 (its bar): views 2.47e-14 at S = 9416 -> 2.2e-14 (7.0e-13); volume 3.12e-15 at
    S = 4000 -> 9.6e-15 (2.1e-13); gated 7.72e-15 at S = 4000 -> 2.7e-14 (5.2e-13).  Twist 6e-15 and node DQs 3e-15 from the oracle."""
    run_case(name, 4, np.float32, S, stride)


def test_rigid_mode_rows_past_the_first_pass_knn8_float64_views():
    """The variant with the most registers: knn = 8 and float64 depth maps, through the views; two passes, the last tile one sample.
    Measured: deviation of the sums 2.27e-14 at S = 9416 -> 5.2e-14 at S = 262 017 (bar 6.4e-13)."""
    run_case("views", 8, np.float64, S_MULTI, 1)


def test_built_rigid_step_past_256_nodes():
    """dfh_gn_global_step (gn_global_step_kernel): 64 workgroups of 4 waves; wave w adds the blocks w, w + 256, ... (lanes 0 .. 35)
    and the right-hand sides of the nodes w, w + 256, ... (lanes 36 .. 41).  The blocks' loop turns many times in every test of
    the step; the nodes' loop never did (at most 216 nodes).  The R = 96 scene with 320 nodes, the regulariser off: the built
    system holds the sums of the sampled step, so the oracle is oracle/gn_np.global_step_sampled at the bars of
    tests/test_gpu_configs.py::test_rigid_mode_step_variants_and_oracle (twist to 1e-9 relative, node DQs to 1e-9).  On the CPU:
    without the right-hand sides of the nodes 256 .. 319 the oracle's twist moves by more than 100 bars."""
    s = _rigid_scene()
    R, N, WAVES = s["R"], 320, 64 * 4
    K, Kinv, scale, center, lws = s["K"], s["Kinv"], s["scale"], s["center"], s["lws"]
    node_pos, node_w = scene.fibonacci_nodes(N, R)
    ident = np.tile(IDENT, (N, 1))
    fs = FrameSolver(K, scale, center, R / 2, knn=4, pcg_iters=10, distributed=False)
    fs.set_graph(node_pos, ident, node_w)
    assert fs.set_canonical(s["T"], s["Wt"], band=2.0) > 5000 and N > WAVES
    sv = fs.solver
    pos, nrm, nbr = sv.spos.cpu().numpy(), sv.snrm.cpu().numpy(), sv.snbr.cpu().numpy().astype(np.int64)
    lives = [d.astype(np.float32) for d in s["live64"]]
    depths = [torch.from_numpy(d).cuda() for d in lives]
    dq0 = G.apply_twists(ident, np.random.default_rng(5).normal(scale=[1e-3] * 3 + [0.1] * 3, size=(N, 6)))

    def assoc(w):
        return G.associate_depth_views(w, K, Kinv, lws, lives, scale, center, R / 2, 2.0)[:2]
    sv.node_dq.copy_(torch.from_numpy(dq0).cuda())
    fs.global_iteration(depths, lws, rw=0.0, max_dist=2.0, huber=HUBER, lm_rel=LM_REL, n_iters=1, built=True)
    xi = sv.global_xi.cpu().numpy()[:6]
    dq = sv.node_dq.cpu().numpy()
    dq_o, xi_o, n_o = G.global_step_sampled(dq0, pos, nrm, nbr, node_pos, node_w, IDENT, assoc, HUBER, LM_REL, stride=1)
    print("valid", n_o, "max |xi - oracle|", float(np.abs(xi - xi_o).max()), "max |dq - oracle|", float(np.abs(dq - dq_o).max()))
    assert n_o > 1000 and np.linalg.norm(xi_o[3:]) > 0.01
    assert np.abs(xi - xi_o).max() <= 1e-9 * max(1.0, np.abs(xi_o).max()), (xi, xi_o)
    assert np.abs(dq - dq_o).max() <= 1e-9
    # what the second turn of the nodes' loop adds: the oracle's g_g without the nodes >= 256
    warped = O.warp(pos, dq0[nbr], node_pos[nbr], node_w[nbr], m_lw=IDENT)
    corr, valid = assoc(warped)
    sel = np.flatnonzero(valid)
    r, J = G.data_residual_jacobian(dq0, pos[sel], nrm[sel], corr[sel], nbr[sel], node_pos, node_w, IDENT)
    sc, _ = G.huber_scale(r, HUBER)
    r, J = r * sc, J * sc[:, None, None]
    Jg = J.sum(axis=1)
    A = Jg.T @ Jg
    A = A + LM_REL * np.diag(np.diag(A))
    late = nbr[sel] >= WAVES                                           # (n, k): the blocks of a node a wave reaches in its second turn
    g_first = np.einsum("nkc,n->c", np.where(late[:, :, None], 0.0, J), r)
    assert np.abs(-np.linalg.solve(A, Jg.T @ r) - xi_o).max() <= 1e-12 * max(1.0, np.abs(xi_o).max())
    moved = float(np.abs(-np.linalg.solve(A, g_first) - xi_o).max())
    print("rows that touch a node >= 256:", int(late.any(axis=1).sum()), "the twist without those nodes moves by", moved)
    assert moved >= 100 * 1e-9 * max(1.0, np.abs(xi_o).max())
