"""Per-frame orchestration of the hot path: surface samples from the canonical volume, their
node neighbourhoods, then GN iterations (associate -> build -> all-reduce -> PCG -> update), then
the TSDF update.  Mirrors the reference's frame loop (test.py:116-131: setupCorrespondences ->
solve -> updateTSDF) with projective association in place of marching cubes + KD-tree.

`extract_surface_samples` runs the HIP band-compaction kernels of csrc/dfh_extract.hip (the
first "next" row of SURVEY.md §8(f)); `extract_surface_samples_torch` is the same computation on
torch ops, kept for CPU-side tests of the sample definition."""
import numpy as np
import torch

from . import _lib, kernels
from .device import HostScalar, current_stream_ptr, dtype_code, require_gpu
from .solve import WarpSolver, relax_twists, sample_knn, warp_points


def extract_surface_samples(T, Wt, band, x0=0, max_samples=None):
    """Band voxels (w > 0, |T| < band; T in voxel units as fuseDepths stores it) of a slab starting
    at global plane x0 -> (surface points (S,3) in global index space, unit normals), fp64 CUDA
    tensors in voxel order.  Three HIP launches (count, scan, emit) and one 8-byte read-back of the
    sample count.  max_samples < the number of band voxels keeps an even subsample in voxel order (sample i iff it is the
    first one with slot floor(i * max_samples / n)), i.e. the whole surface at a lower density, never a prefix."""
    require_gpu()
    lib = _lib.load()
    if not (isinstance(T, torch.Tensor) and T.is_cuda and T.dim() == 3 and T.is_contiguous() and Wt.shape == T.shape
            and Wt.is_cuda and Wt.is_contiguous() and Wt.dtype == T.dtype):
        raise ValueError("T and Wt must be contiguous 3-D CUDA tensors of the same shape and dtype")
    res = _lib.iarr(T.shape)
    nbytes = lib.dfh_surface_workspace_bytes(res)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=T.device)
    total = HostScalar(torch.int64)                    # (the scan kernel stores the count straight into pinned host memory)
    _lib.check(lib.dfh_surface_count(T.data_ptr(), Wt.data_ptr(), dtype_code(T), res, float(band), ws.data_ptr(),
                                     ws.numel() * 8, total.ptr(), current_stream_ptr()), "dfh_surface_count")
    n = total.get()
    cap = n if max_samples is None else min(n, int(max_samples))
    pos = torch.empty((cap, 3), dtype=torch.float64, device=T.device)
    nrm = torch.empty((cap, 3), dtype=torch.float64, device=T.device)
    _lib.check(lib.dfh_surface_emit(T.data_ptr(), Wt.data_ptr(), dtype_code(T), res, int(x0), float(band), ws.data_ptr(),
                                    pos.data_ptr(), nrm.data_ptr(), cap, current_stream_ptr()), "dfh_surface_emit")
    return pos, nrm


def extract_surface_samples_torch(T, Wt, band, x0=0, max_samples=None):
    """Same samples on torch ops (works on CPU tensors).  Band voxels of a slab
    starting at global plane x0 -> (surface points (S,3) in global index space, unit normals).
    Normals are central differences of T inside the slab (one-sided at its faces); points are the
    voxel centres moved onto the zero level set by one Newton step, centre - T grad / |grad|^2, of length <= |T|."""
    Tf = T.to(torch.float64)
    mask = (Wt > 0) & (Tf.abs() < band)
    idx = mask.nonzero(as_tuple=False)
    if max_samples is not None and idx.shape[0] > max_samples:
        n, cap = idx.shape[0], int(max_samples)                  # the device rule: first sample of every slot floor(i * cap / n)
        idx = idx[(torch.arange(cap, device=idx.device, dtype=torch.int64) * n + cap - 1) // cap]
    X, Y, Z = T.shape
    ix, iy, iz = idx[:, 0], idx[:, 1], idx[:, 2]

    def diff(axis_idx, n, take):
        lo, hi = (axis_idx - 1).clamp(min=0), (axis_idx + 1).clamp(max=n - 1)
        return (take(hi) - take(lo)) / (hi - lo).clamp(min=1).to(torch.float64)      # (a one-voxel-thick axis: 0 / 1, as the kernels)
    gx = diff(ix, X, lambda a: Tf[a, iy, iz])
    gy = diff(iy, Y, lambda a: Tf[ix, a, iz])
    gz = diff(iz, Z, lambda a: Tf[ix, iy, a])
    g = torch.stack([gx, gy, gz], dim=1)
    nrm = g.norm(dim=1, keepdim=True)
    ok = (nrm[:, 0] > 1e-6) & torch.isfinite(nrm[:, 0])          # finite and > 1e-6: a NaN or infinite neighbour yields no sample
    idx, g, nrm = idx[ok], g[ok], nrm[ok]
    n = g / nrm
    pos = idx.to(torch.float64)
    pos[:, 0] += x0
    pos = pos - (Tf[idx[:, 0], idx[:, 1], idx[:, 2]][:, None] / nrm.clamp(min=1.0)) * n   # one Newton step: T grad / |grad|^2, no longer than |T|
    return pos.contiguous(), n.contiguous()


class FrameSolver:
    """Warp-field estimation of one live depth frame against the canonical volume."""

    def __init__(self, K, scale, center, half, knn=4, pcg_iters=10, distributed=True):
        self.K = np.asarray(K, dtype=np.float64)
        self.Kinv = np.linalg.inv(self.K)
        self.scale, self.center, self.half = float(scale), np.asarray(center, dtype=np.float64), float(half)
        self.solver = WarpSolver(knn=knn, pcg_iters=pcg_iters, distributed=distributed)
        self.knn = knn
        self.lw = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])

    def set_graph(self, node_pos, node_dq, node_w):
        node_nbr, _ = sample_knn(node_pos, node_pos, node_w, self.knn)        # a node's own k nearest nodes
        self.solver.set_graph(node_pos, node_dq, node_w, node_nbr=node_nbr)

    def set_landmarks(self, pos, target, conf=None, weight=1.0, huber=0.0, max_dist=0.0):
        """The landmark term of the solve (WarpSolver.set_landmarks): canonical points `pos` with live 3-D targets `target`, both in
        index space, as three point-to-point rows each of weight `weight` (x conf), with the vector Huber delta `huber` and the
        gate `max_dist` on |x' - c| in voxels.  Every build of this solver adds them until clear_landmarks() or a new graph."""
        sv = self.solver
        sv.landmark_weight, sv.landmark_huber, sv.landmark_max_dist = float(weight), float(huber), float(max_dist)
        sv.set_landmarks(pos, target, conf=conf)

    def clear_landmarks(self):
        self.solver.clear_landmarks()

    def landmarks_active(self):
        """True while the builds add a landmark term."""
        sv = self.solver
        return sv._lm is not None and sv._lm["L"] > 0 and float(sv.landmark_weight) != 0.0

    def set_photometric(self, ref, valid=None, conf=None, weight=1e-3, huber=0.0, max_diff=0.0, band_sd=float("inf"), presorted=False):
        """The photometric term of the solve (WarpSolver.set_photometric): a reference intensity `ref` (0..255) per sample, compared
        with the colour images a gn_iteration / global_iteration is given (colors=) as one row per sample of weight `weight`
        (x conf), with the Huber delta `huber` and the gate `max_diff` on |I - ref| (intensity units) and the depth gate `band_sd` on
        |sd| (the depth maps' units).  Until clear_photometric(), new samples or a new graph."""
        sv = self.solver
        sv.photo_weight, sv.photo_huber, sv.photo_max_diff, sv.photo_band_sd = float(weight), float(huber), float(max_diff), float(band_sd)
        sv.set_photometric(ref, valid=valid, conf=conf, presorted=presorted)

    def clear_photometric(self):
        self.solver.clear_photometric()

    def photometric_active(self):
        """True while the builds that are given colour images add a photometric term."""
        sv = self.solver
        return sv._ph is not None and sv.S > 0 and float(sv.photo_weight) != 0.0

    def set_canonical(self, T, Wt, band=1.0, x0=0, max_samples=None, knn_bricks=None):
        """knn_bricks: see solve.sample_knn (candidate lists of the K3 workspace: the samples' node search skips its
        per-workgroup bounding-box pass)."""
        pos, nrm = extract_surface_samples(T, Wt, band, x0=x0, max_samples=max_samples)
        self.solver.set_samples(pos, nrm, knn_bricks=knn_bricks)
        return pos.shape[0]

    def gn_iteration(self, depth, lw_cam, rw=5.0, lm_abs=10.0, lm_rel=1e-2, max_dist=2.0, huber=0.0, n_iters=1, n_global=0, global_lm=0.1,
                     normals=None, normal_cos=0.5, colors=None):
        """associate -> build (+ all-reduce) -> PCG -> twist update, n_iters times; asynchronous.  depth / lw_cam may be lists
        (several live views: every sample associates with the view in which it lies closest to the observed surface).
        n_global: that many rigid-mode steps first (global_iteration), in the same library call on one GPU.
        normals / normal_cos: the normal gate of WarpSolver.associate_depth ((V, H, W, 3) float32 live normal maps; None: none).
        colors: one colour image per depth map: every build adds the photometric term (set_photometric)."""
        kw = {} if colors is None else {"colors": colors}
        self.solver.iterate_associated(depth, self.K, self.Kinv, lw_cam, self.scale, self.center, self.half, self.lw, rw, max_dist, huber,
                                       lm_abs, lm_rel, n_iters=n_iters, n_global=n_global, global_lm=global_lm, normals=normals,
                                       normal_cos=normal_cos, **kw)

    def global_iteration(self, depth, lw_cam, rw=5.0, max_dist=2.0, huber=0.0, lm_rel=0.1, n_iters=1, built=False, stride=1,
                         normals=None, normal_cos=0.5, colors=None):
        """The rigid mode alone -- one twist shared by all nodes -- n_iters times; asynchronous.  Worth several node iterations where
        the live frame has moved as a whole: ten truncated PCG iterations hardly touch that mode.  Default: straight from the
        samples (WarpSolver.global_sampled: data rows only, two short launches a step); built=True: from the built normal
        equations, regulariser included (associate -> build (+ all-reduce) -> WarpSolver.global_step).
        normals / normal_cos: the normal gate of WarpSolver.associate_depth, on either route.
        colors: built=True only: the builds add the photometric term (the sampled steps read data rows only and refuse them)."""
        if not built and colors is not None:
            raise ValueError("colors= needs built=True: the sampled rigid-mode steps read the data rows only")
        if not built:
            self.solver.global_sampled(depth, self.K, self.Kinv, lw_cam, self.scale, self.center, self.half, self.lw, max_dist, huber, lm_rel,
                                       n_steps=n_iters, stride=stride, normals=normals, normal_cos=normal_cos)
            return
        for _ in range(int(n_iters)):
            self.solver.build_associated(depth, self.K, self.Kinv, lw_cam, self.scale, self.center, self.half, self.lw, rw, max_dist, huber,
                                         normals, normal_cos, **({} if colors is None else {"colors": colors}))
            self.solver.global_step(lm_rel)

    def gn_iteration_volume(self, live, band, rw=5.0, lm_abs=10.0, lm_rel=1e-2, max_dist=2.0, huber=0.0, n_iters=1, min_grad=0.5,
                            value_to_vox=1.0):
        """gn_iteration with the volume data term: associate against the live TSDF volume inside the build
        (WarpSolver.build_volume; + all-reduce) -> PCG -> twist update, n_iters times, in one library call on one GPU
        (WarpSolver.iterate_volume); asynchronous."""
        self.solver.iterate_volume(live, self.lw, rw, band, max_dist, huber, lm_abs, lm_rel, n_iters=n_iters, n_global=0,
                                   min_grad=min_grad, value_to_vox=value_to_vox)

    def global_iteration_volume(self, live, band, rw=5.0, max_dist=2.0, huber=0.0, lm_rel=0.1, n_iters=1, min_grad=0.5, value_to_vox=1.0,
                                built=True, stride=1):
        """The rigid mode alone with the volume data term, n_iters times; asynchronous.  built=True (the default): from the built
        normal equations, regulariser included (associate against the volume inside the build (+ all-reduce) ->
        WarpSolver.global_step).  built=False: straight from the samples of every `stride`-th tile
        (WarpSolver.global_sampled_volume: data rows only, no build, no gather)."""
        if not built:
            self.solver.global_sampled_volume(live, self.lw, band, max_dist, huber, lm_rel, n_steps=n_iters, stride=stride,
                                              min_grad=min_grad, value_to_vox=value_to_vox)
            return
        self.solver.iterate_volume(live, self.lw, rw, band, max_dist, huber, n_iters=0, n_global=n_iters, global_lm=lm_rel,
                                   min_grad=min_grad, value_to_vox=value_to_vox)

    def solve(self, depth, lw_cam, rw=5.0, iters=10, **kw):
        costs = []
        for _ in range(iters):
            self.gn_iteration(depth, lw_cam, rw, **kw)
            costs.append(self.solver.cost())
        return costs


class SlabFrame:
    """One rank's share of the per-frame loop (reference test.py:116-131) with the canonical volume cut into
    axis-0 slabs: live depth -> this rank's live slab (K1, no exchange) -> all-gather of the live volume ->
    GN iterations (samples of this slab; one all-reduce of the normal equations per iteration) -> canonical
    slab <- live volume through the warp field (K3) -> this slab's samples for the next frame.
    With one rank it is the single-GPU frame.
    The deformation graph comes from outside (node_pos, node_w) or, with node_pos = node_w = None, from the loop's own
    volume: integrate() the initial views, then construct_graph(radius)."""

    RELAX = 0.8          # default of step(relax=...): see there
    GLOBAL_ITERS = 2     # default of step(global_iters=...): rigid-mode steps in front of the node iterations
    GLOBAL_STRIDE = 4    # ... each fitted to every 4th 128-sample tile (step(global_stride=...))
    has_graph = False    # set by the constructor (node_pos given) or by construct_graph()
    SAMPLE_SOURCES = ("band", "visible")
    sample_source = "band"   # set_sample_source(): where refresh_samples() takes the solve's samples from

    def __init__(self, K, scale, center, res, tdist_vox, node_pos, node_w, knn=4, pcg_iters=10, band=4.0, volume_dtype=torch.float32,
                 distributed=True, solve_mode="auto", depth_prep=None, normal_gate=None, color_band=None, photo_weight=0.0,
                 photo_huber=0.0, photo_max_diff=0.0, photo_band_sd=None, ingest=None, tracker=None, track_model="live"):
        """tracker: a tracking.CameraTracker, or None.  step(track=True) then treats the given lw_cam as a PRIOR: the frame's depth
        maps (after ingest and depth_prep) are aligned to the model as the prior cameras see it, and the tracked cameras replace
        lw_cam before anything else reads it; they are kept in `self.tracked_lw`, the tracker's report in `self.track_stats` (a
        lost view keeps its prior).  track_model: what the model is.  "live" = raycast_live: the previous frame's live volume --
        it needs a previous step() that swept one, and works on several ranks: every rank casts the same gathered volume and the
        tracker's sums are order-fixed, so every rank computes identical poses and no collective is added.  "mesh" = render_live:
        the canonical model warped by the current field, single rank only; its rendered normals are not turned to face the
        camera, so this model tracks without the normal-compatibility gate.  Views are tracked independently.
        ingest: an ingest.RGBDIngest, or None.  step() and integrate() then take the sensor's RAW frames -- uint16 depth maps,
        one per calibrated view, and (step) the colour camera's raw images -- and run them through the stage first, in front of
        depth_prep: its depth maps go to everything that read depth before, its registered colours with the depth maps that keep
        only coloured pixels (`self.color_depth`) to the colour fusion.  The photometric term keeps the frame's depth maps and the
        registered colours: a pixel without a valid colour reaches it as RGB 0, which is what photo_max_diff is for.  `K` must
        equal ingest.K, the pinhole the stage resamples to.  The stage's outputs (`self.ingest_depth`, `self.ingest_color`,
        `self.color_depth`) are rewritten in place by the next call.
        photo_weight: > 0 switches the photometric term of the solve on (FrameSolver.set_photometric); it needs color_band.  After
        every sample refresh the samples' reference intensities are the luma of the colour volume at their canonical positions
        (kernels.sample_colors; samples the volume has no colour for get no row), and the next step(colors=...) compares them with
        that frame's colour images in every build of its solve (the depth data term) -- before the images are fused, which is
        step()'s order anyway.  While it is on, the rigid-mode steps come from the built system, as with landmarks.  photo_huber /
        photo_max_diff: the Huber delta and the gate on |I - ref| in intensity units (0: none); photo_band_sd: the depth gate on |sd|
        in the depth maps' units (default color_band * |scale|, the colour fusion's).  Single rank only.
        color_band: None, or the half-width in voxels of the canonical band that takes colour: a number allocates the colour
        volume `self.C` of this rank's slab (kernels.color_volume) and step(colors=...) fuses each frame's colour images into it.
        normal_gate: None, or the smallest cosine between a sample's warped normal and the live normal of the pixel it is matched
        to that still gives a correspondence (the normal gate of the depth data term, WarpSolver.associate_depth; 0.5 = 60 degrees):
        step() then passes this frame's live normal maps to the rigid-mode steps and the node iterations.  It needs depth_prep
        (where the normal maps come from) and data_term="depth"; step(normal_gate=...) overrides it per call.  The normal maps are a
        per-frame input on every rank, so several ranks need nothing further (that case has not been measured).
        depth_prep: a depth_prep.DepthPrep, or None.  step() then cleans the frame's depth maps once, before anything reads
        them (the live sweep, the solve's association, an update="depth" fusion), and keeps the cleaned maps in
        `self.clean_depth` (list of (H, W) float32 views) and the live normal maps in `self.live_normals` ((V, H, W, 3)) for the
        caller; both are rewritten in place by the next step() with maps of the same number and size.
        solve_mode (several ranks): "sharded" = every rank builds the normal equations of its own slab's samples, one
        all-reduce per GN iteration (BASELINE north star); "replicated" = the slabs' samples are all-gathered once per frame
        and every rank solves the whole system, no per-iteration collective (bit-identical warp fields on all ranks, and the
        single-GPU loop's bits WHEN both run the same PCG path -- _lib dfh_pcg_path: ranks that share one GPU, a rehearsal, take
        the two-launch kernels, one rank per GPU the persistent kernel like a single-GPU run; tests/test_gpu_dist_gloo.py pins it at
        256^3 / 512 nodes); "auto" = dist.solve_mode's latency model, decided at the first sample refresh."""
        from . import dist as D
        self.D = D
        self.distributed = bool(distributed)
        if solve_mode not in ("auto", "sharded", "replicated"):
            raise ValueError("solve_mode must be 'auto', 'sharded' or 'replicated'")
        self.solve_mode = solve_mode
        self.R = int(res)
        self.K = np.asarray(K, dtype=np.float64)
        self.Kinv = np.linalg.inv(self.K)
        self.scale, self.center, self.tvox = float(scale), np.asarray(center, dtype=np.float64), float(tdist_vox)
        self.tdist_world = self.tvox * self.scale
        self.rank, self.ws = D.world() if self.distributed else (0, 1)     # distributed=False: the whole grid, no collectives
        self.a, self.b = D.slab_range(self.R, self.rank, self.ws)
        R = self.R
        self.T = torch.full((self.b - self.a, R, R), self.tvox, dtype=volume_dtype, device="cuda")
        self.Wt = torch.zeros_like(self.T)
        self.live = torch.empty_like(self.T)
        self.live_w = torch.empty_like(self.T)
        self.band, self.knn = float(band), int(knn)
        self.color_band = None if color_band is None else float(color_band)
        if self.color_band is not None and not self.color_band > 0.0:
            raise ValueError("color_band must be None or > 0, got %r" % (color_band,))
        self.C = None if self.color_band is None else kernels.color_volume((R, R, R), (self.a, self.b))
        self.photo_weight, self.photo_huber, self.photo_max_diff = float(photo_weight), float(photo_huber), float(photo_max_diff)
        if not self.photo_weight >= 0.0:
            raise ValueError("photo_weight must be >= 0, got %r" % (photo_weight,))
        if self.photo_weight > 0.0 and self.ws > 1:
            raise ValueError("the photometric term (photo_weight > 0) is single-rank only: %d ranks" % self.ws)
        if self.photo_weight > 0.0 and self.color_band is None:
            raise ValueError("photo_weight > 0 needs color_band: the reference intensities come from the colour volume")
        self.photo_band_sd = None if photo_band_sd is None else float(photo_band_sd)
        self.photo_active = None                 # after a step() whose solve had colour rows: uint8 per sample of that solve (the
                                                 # solver's order then), 1 = the row was active in its last build
        # (replicated / undecided: the solver itself runs no collective; a decision for "sharded" switches it on)
        self.fs = FrameSolver(K, scale, center, R / 2, knn=knn, pcg_iters=pcg_iters,
                              distributed=self.distributed and self.ws > 1 and solve_mode == "sharded")
        if (node_pos is None) != (node_w is None):
            raise ValueError("node_pos and node_w come together (both None: construct_graph() builds the graph)")
        if track_model not in ("live", "mesh"):
            raise ValueError("track_model must be 'live' or 'mesh', got %r" % (track_model,))
        self.tracker, self.track_model = tracker, track_model
        self.tracked_lw = self.track_stats = None
        self.ingest = ingest
        if ingest is not None and not np.array_equal(self.K, np.asarray(ingest.K, dtype=np.float64)):
            raise ValueError("K must equal ingest.K: the stage resamples every depth map to that pinhole")
        self.ingest_depth = self.ingest_color = self.color_depth = None
        self._ingest_out = None                  # the stage's output buffers, reused from frame to frame
        self.depth_prep = depth_prep
        self.normal_gate = self._check_normal_gate(normal_gate, depth_prep)
        self.clean_depth = self.live_normals = None
        self._prep_out = None                    # step()'s output buffers of depth_prep, reused from frame to frame
        self.ws_views = None                     # the multi-view dfh_integrate_depth's scratch (parameters + depth pyramids): sized on first use
        self._side = None                        # side stream of step(): the live-volume sweep beside the plan build
        self.updated = None                      # event recorded by step() right after the TSDF update
        self.ws_dqb = None
        self.knn_bricks = None
        self._first = True
        self.ident_lw = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
        self._landmarks = None                   # set_landmarks()'s arguments: handed to the solver again after a graph change
        self.has_graph = node_pos is not None    # False: everything that depends on the graph waits for construct_graph()
        if self.has_graph:
            N = len(node_pos)
            ident = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0, 0]), (N, 1))
            self.fs.set_graph(node_pos, ident, node_w)
            self._graph_workspaces(node_pos, N)

    def set_landmarks(self, canon_pos, target, conf=None, weight=1.0, huber=0.0, max_dist=0.0):
        """Feature correspondences as 3-D constraints of every following step()'s solve (FrameSolver.set_landmarks): canonical
        points `canon_pos` (L, 3) and their live targets (L, 3) in index space, conf (L,) optional.  They survive the sample refresh
        at the end of a step and are handed to the solver again when the graph changes (construct_graph, update_graph: their
        node tuples are searched anew).  While they are set, the rigid-mode steps of step() come from the BUILT system (the sampled
        steps read the data rows only and would not see them).  Every rank passes the same landmarks."""
        self._landmarks = (canon_pos, target, conf, float(weight), float(huber), float(max_dist))
        if self.has_graph:
            self.fs.set_landmarks(*self._landmarks)

    def clear_landmarks(self):
        self._landmarks = None
        self.fs.clear_landmarks()

    def _set_graph(self, node_pos, node_dq, node_w):
        """FrameSolver.set_graph, then the landmarks again (a new graph drops the solver's: their node tuples were the old graph's)."""
        self.fs.set_graph(node_pos, node_dq, node_w)
        if self._landmarks is not None:
            self.fs.set_landmarks(*self._landmarks)

    @staticmethod
    def _check_normal_gate(normal_gate, depth_prep):
        """A normal gate's value: None, or a cosine in [0, 1] together with a depth_prep (the source of the live normals)."""
        if normal_gate is None:
            return None
        cos = float(normal_gate)
        if not 0.0 <= cos <= 1.0:
            raise ValueError("normal_gate must be None or a cosine in [0, 1], got %r" % (normal_gate,))
        if depth_prep is None:
            raise ValueError("normal_gate needs depth_prep: the live normal maps come from there")
        return cos

    _KEEP = object()          # step(normal_gate=...): "the constructor's value"

    def _graph_workspaces(self, node_pos, N):
        """K3's workspace and the per-brick candidate lists for a graph of N nodes (the samples' node search uses the same lists)."""
        R = self.R
        self.ws_dqb = kernels.dqb_workspace((R, R, R), (self.a, self.b), knn=self.knn, n_nodes=N)
        self.knn_bricks = None
        if self.b > self.a:
            kernels.dqb_build_candidates(self.ws_dqb, (R, R, R), node_pos, self.knn, (self.a, self.b))
            self.knn_bricks = ((R, R, R), (self.a, self.b), self.ws_dqb)
        self._first = True                               # K3 stores its per-voxel neighbourhoods again on the next call

    def _ingest(self, raw_depths, raw_colors):
        """The ingest stage on one frame's raw maps (and images): (list of depth maps, list of registered colour images or None,
        list of colour-only depth maps or None), views of buffers the next call rewrites."""
        V = len(raw_depths)
        have = self._ingest_out
        if have is None or have[0].shape[0] != V or (raw_colors is not None and have[1] is None):
            have = None
        d, c, cd = self.ingest(raw_depths, raw_colors, out=None if have is None else (have[0], have[1] if raw_colors is not None else None,
                                                                                      have[2] if raw_colors is not None else None))
        if have is None:
            self._ingest_out = (d, c, cd)
        self.ingest_depth, self.ingest_color, self.color_depth = d, c, cd
        return [d[v] for v in range(V)], None if c is None else [c[v] for v in range(V)], None if cd is None else [cd[v] for v in range(V)]

    def integrate(self, depth, lw_cam):
        """Fuse a depth map into this rank's canonical slab (initial frames).  With the constructor's ingest: `depth` is the
        frame's raw uint16 maps, one per calibrated view, and lw_cam their extrinsics (lists; a single map for a one-view rig)."""
        R = self.R
        if self.ingest is not None:
            raw = list(depth) if isinstance(depth, (list, tuple)) else [depth]
            lws = list(lw_cam) if isinstance(depth, (list, tuple)) else [lw_cam]
            if len(raw) != len(lws):
                raise ValueError('length of camera matrix array must equal that of depth maps')
            for d, lw in zip(self._ingest(raw, None)[0], lws):
                kernels.integrate_depth(self.T, self.Wt, d, self.K, self.Kinv, lw, self.scale, self.center, self.tdist_world,
                                        tsdf_res=R, res=(R, R, R), x_range=(self.a, self.b))
            return
        kernels.integrate_depth(self.T, self.Wt, depth, self.K, self.Kinv, lw_cam, self.scale, self.center, self.tdist_world,
                                tsdf_res=R, res=(R, R, R), x_range=(self.a, self.b))

    def _slab_with_halo(self):
        """This rank's slab with its neighbours' face planes at weight 0 (see refresh_samples) -> (T, Wt, first global plane)."""
        lo, hi = self.D.halo_planes(self.T, self.R)
        Tp, Wp, x0 = [self.T], [self.Wt], self.a
        if lo is not None:
            Tp.insert(0, lo[None]); Wp.insert(0, torch.zeros_like(lo)[None]); x0 -= 1
        if hi is not None:
            Tp.append(hi[None]); Wp.append(torch.zeros_like(hi)[None])
        return torch.cat(Tp).contiguous(), torch.cat(Wp).contiguous(), x0

    def band_samples(self):
        """The band samples of this rank's slab (positions in global index space, unit normals; CUDA fp64, voxel order): the
        bare extraction of refresh_samples(), which needs no graph."""
        if self.ws == 1:
            return extract_surface_samples(self.T, self.Wt, self.band, x0=self.a)
        Tp, Wp, x0 = self._slab_with_halo()
        return extract_surface_samples(Tp, Wp, self.band, x0=x0)

    @staticmethod
    def _canonical_order(pts):
        """Rows of a (n,3) tensor sorted by x, then y, then z -- np.lexsort((z, y, x)) as three stable sorts on the tensor's device."""
        o = torch.sort(pts[:, 2], stable=True).indices
        o = o[torch.sort(pts[o, 1], stable=True).indices]
        o = o[torch.sort(pts[o, 0], stable=True).indices]
        return pts[o]

    def construct_graph(self, radius, sampler="device"):
        """The deformation graph from the loop's own canonical volume (after the initial integrate() calls): the band samples of
        all slabs, ordered canonically by position (so the graph does not depend on the slab partition), radius-subsampled
        (graph.uniform_sample_device, or graph.uniform_sample with sampler="host": the same nodes) into nodes with identity
        DQs and weight 2 * radius (core/fusion.py:116); the solver's graph, K3's workspace and candidate lists and the samples
        are then set up as update_graph() does after an insertion.  Returns the node count."""
        from . import graph as _graph
        _graph._check_sampler(sampler)
        radius = float(radius)
        if not (np.isfinite(radius) and radius > 0):
            raise ValueError("construct_graph needs a finite radius > 0")
        pts, _ = self.band_samples()
        if self.ws > 1:
            pts = self.D.gather_rows(pts)
        pts = self._canonical_order(pts)
        if sampler == "device":
            nodes, _ = _graph.uniform_sample_device(pts, radius)
        else:
            nodes, _ = _graph.uniform_sample(pts.cpu().numpy(), radius)
            nodes = _graph._dev64(np.asarray(nodes, dtype=np.float64).reshape(-1, 3))
        N = int(nodes.shape[0])
        if N < self.knn:
            raise ValueError("construct_graph: %d band samples gave %d nodes, fewer than knn = %d" % (pts.shape[0], N, self.knn))
        ident = torch.zeros((N, 8), dtype=torch.float64, device="cuda")
        ident[:, 0] = 1.0
        self._set_graph(nodes, ident, torch.full((N,), 2.0 * radius, dtype=torch.float64, device="cuda"))
        self.has_graph = True
        self._graph_workspaces(nodes, N)
        self.refresh_samples()
        return N

    def refresh_samples(self):
        """_refresh_samples, then (photo_weight > 0) the new samples' reference intensities from the colour volume."""
        n = self._refresh_samples()
        self._refresh_photo()
        return n

    def _refresh_photo(self):
        """The photometric term's reference intensities for the solver's current samples: the luma of the colour volume at their
        canonical positions, valid where the volume has colour.  Nothing while photo_weight is 0."""
        if not self.photo_weight > 0.0:
            return
        sv = self.fs.solver
        if sv.S == 0:
            sv.clear_photometric()
            return
        rgb, valid = kernels.sample_colors(self.C, sv.spos)
        rgb = rgb.double()
        ref = (77.0 * rgb[:, 0] + 150.0 * rgb[:, 1] + 29.0 * rgb[:, 2]) / 256.0
        band_sd = self.color_band * abs(self.scale) if self.photo_band_sd is None else self.photo_band_sd
        self.fs.set_photometric(ref, valid=valid, weight=self.photo_weight, huber=self.photo_huber, max_diff=self.photo_max_diff,
                                band_sd=band_sd, presorted=True)

    def _refresh_samples(self):
        """Samples of this slab.  Normals are central differences of T, also across the slab faces: the
        neighbours' face planes come as a halo whose weight is 0 (they feed gradients, never samples), so the
        union over ranks is exactly the whole-grid sample set."""
        if not self.has_graph:
            raise ValueError("no deformation graph yet: call construct_graph() first (band_samples() needs none)")
        if self.sample_source == "visible":
            # the rendered model is the sample set (set_sample_source); none visible is a valid state: S = 0, the solve a no-op
            pos, nrm, _ = self.visible_samples(self._src_lws, self._src_size[0], self._src_size[1], stride=self._src_stride,
                                               max_samples=self._src_max)
            self.fs.solver.set_samples(pos, nrm, knn_bricks=self.knn_bricks)
            return int(pos.shape[0])
        if self.ws == 1:
            return self.fs.set_canonical(self.T, self.Wt, band=self.band, x0=self.a, knn_bricks=self.knn_bricks)
        Tp, Wp, x0 = self._slab_with_halo()
        if self.solve_mode == "sharded":
            return self.fs.set_canonical(Tp, Wp, band=self.band, x0=x0, knn_bricks=self.knn_bricks)
        # replicated (or still to be decided): this slab's samples with their node tables, then all slabs' in rank order --
        # the whole-grid sample set in the whole-grid order (slabs are x ranges, samples are emitted x-major)
        sv = self.fs.solver
        pos, nrm = extract_surface_samples(Tp, Wp, self.band, x0=x0)
        nbr, wts = sample_knn(pos, sv.node_pos, sv.node_w, self.knn, bricks=self.knn_bricks) if pos.shape[0] else \
            (torch.empty((0, self.knn), dtype=torch.int32, device="cuda"), torch.empty((0, self.knn), dtype=torch.float64, device="cuda"))
        packed = torch.cat([pos, nrm, wts, nbr.to(torch.float64)], dim=1)        # (node indices are exact in fp64)
        dev = self.D.collective_device()
        allp = self.D.allgather_ragged(packed.to(dev)).to("cuda")
        k = self.knn
        if self.solve_mode == "auto":
            S_all, N = int(allp.shape[0]), int(sv.N)
            mode = self.D.solve_mode(S_all, N, 12 * N, self.ws)               # (~11.5 blocks per node row in practice)
            self.solve_mode = mode
            if mode == "sharded":                                             # every rank decides alike: same inputs
                self.fs.solver.distributed = True
                return self.fs.set_canonical(Tp, Wp, band=self.band, x0=x0, knn_bricks=self.knn_bricks)
        sv.set_samples(allp[:, 0:3].contiguous(), allp[:, 3:6].contiguous(), nbr=allp[:, 6 + k:6 + 2 * k].to(torch.int32).contiguous(),
                       weights=allp[:, 6:6 + k].contiguous())
        return int(allp.shape[0])

    def update_graph(self, radius=None, sampler="host"):
        """Deformation-graph maintenance after a TSDF update (reference Fusion.update_graph, core/fusion.py:201-239) on the
        device path, with this loop's surface points -- the band samples of the canonical slab -- in the role of the mesh
        vertices: samples no node supports (min over their knn nodes of |node - p| / w >= 1) are radius-subsampled into new
        nodes whose DQs are the blend of the old graph at their positions; the solver's graph, K3's stored neighbourhoods
        and candidate lists and the samples' node table are rebuilt when nodes were inserted.  Every rank inserts the same
        nodes (the unsupported points are gathered in rank order before the greedy subsampling).  Returns the number of
        inserted nodes.  radius defaults to half the nodes' weight (w = 2 radius, core/fusion.py:116).
        sampler="device": the unsupported points stay on the device -- gathered over ranks as tensors, ordered by three stable
        sorts, subsampled by graph.uniform_sample_device; the same nodes as with "host"."""
        from . import graph as _graph
        _graph._check_sampler(sampler)
        if not self.has_graph:
            raise ValueError("no deformation graph yet: call construct_graph() first")
        sv = self.fs.solver
        if radius is None:
            radius = 0.5 * float(sv.node_w[0])
        if self.sample_source == "band":
            pts = sv.spos if sv.S > 0 else torch.zeros((0, 3), dtype=torch.float64, device="cuda")
        else:                                            # the graph must not grow by what the cameras happen to see: the band
            pts, _ = self.band_samples()                 # samples (construct_graph's points), which the solver does not hold now
        gather = None
        if self.ws > 1 and self.solve_mode == "sharded":         # (replicated: every rank already holds every sample)
            def gather(uns):                             # (ragged all-gather on one device: dist.gather_rows)
                return self.D.gather_rows(np.asarray(uns, dtype=np.float64).reshape(-1, 3))
        # the samples are stored sorted by node tuple; the greedy subsampling depends on the order of its input, so it is
        # fed in a canonical order (by position) that does not depend on the slab partition
        def canon(uns):
            if gather is not None:
                uns = gather(uns)
            if len(uns) == 0:
                return uns
            return uns[np.lexsort((uns[:, 2], uns[:, 1], uns[:, 0]))]

        def canon_device(uns):
            if gather is not None:
                uns = self.D.gather_rows(uns)
            return self._canonical_order(uns)
        vidx, P2, Q2, W2, lookup, n_new = _graph.update_graph_device(sv.node_pos, sv.node_dq, sv.node_w, pts, radius, self.knn,
                                                                    gather_unsupported=canon_device if sampler == "device" else canon,
                                                                    sampler=sampler)
        if n_new == 0:
            return 0
        self._set_graph(P2, Q2, W2)                      # resets the block pattern; node-node table of the regulariser rebuilt
        self._graph_workspaces(P2, int(P2.shape[0]))
        self.refresh_samples()
        return n_new

    def render_live(self, lws, H, W, K=None):
        """K: the intrinsics to render through (None: the frame's).  Depth / normal / face-id maps of the loop's current live model in the views `lws` (one 3x4 world->camera matrix or a
        list; one launch): marching cubes of the canonical volume T at level 0, warped by the solver's node field (node_pos /
        node_dq / node_w, each vertex's knn nearest nodes) and the loop's identity `lw`, rendered with this frame's K / scale /
        center / half (mesh.render).  Single rank only: with the volume cut into slabs the meshes would need halo planes and the
        ranks' z-buffers a merge, which is not implemented (ValueError)."""
        if self.ws > 1:
            raise ValueError("render_live renders one rank's whole grid; the %d-rank slab partition is not supported" % self.ws)
        from . import mesh as _mesh
        verts, faces, normals, _ = _mesh.marching_cubes(self.T, 0.0, 1)
        sv = self.fs.solver
        if verts.shape[0] > 0:
            nbr, _ = sample_knn(verts, sv.node_pos, sv.node_w, self.knn)
            verts, normals = warp_points(verts, normals, self.ident_lw, nbr=nbr, node_dq=sv.node_dq, node_pos=sv.node_pos,
                                         node_w=sv.node_w)
        return _mesh.render(verts, faces, normals, self.K if K is None else np.asarray(K, dtype=np.float64), lws, H, W, scale=self.scale,
                            center=self.center, half=self.R / 2)

    _live_views = None       # (lws, H, W) of the last live sweep of step(): raycast_live's default views

    def raycast_live(self, lws=None, H=None, W=None, K=None, **kw):
        """K: the intrinsics to cast through (None: the frame's).  The LIVE volume the last step() swept from its depth maps, ray-cast (kernels.raycast) into the views `lws` -- default:
        that frame's own cameras and map size, so that `.depth` lines up with the frame's depth maps pixel for pixel and goes
        straight into mesh.depth_error(rendered, observed, gate).  No mesh is built; no warp field is involved (the live volume
        is in the live frame already).  Several ranks: every rank casts the all-gathered live volume (one collective per
        call, two with min_weight > 0) and gets the same maps.  **kw goes to kernels.raycast.  Needs a step() that swept the live
        volume (update="volume" or data_term="volume")."""
        if self._live_views is None:
            raise ValueError("no live volume yet: raycast_live needs a step() with update='volume' or data_term='volume'")
        l0, H0, W0 = self._live_views
        lws = l0 if lws is None else ([lws] if np.asarray(lws[0]).ndim == 1 else list(lws))
        H, W = (H0 if H is None else int(H)), (W0 if W is None else int(W))
        R = self.R
        live, live_w = self.live, self.live_w
        if self.ws > 1:
            live = self.D.allgather_planes(self.live, R)
            live_w = self.D.allgather_planes(self.live_w, R) if kw.get("min_weight", 0.0) > 0.0 else live
        x_range = (self.a, self.b) if self.ws == 1 else None
        K, Kinv = (self.K, self.Kinv) if K is None else (np.asarray(K, dtype=np.float64), np.linalg.inv(np.asarray(K, dtype=np.float64)))
        return kernels.raycast(live, live_w, K, Kinv, lws, H, W, self.scale, self.center, tsdf_res=R, res=(R, R, R),
                               x_range=x_range, **kw)

    def raycast_canonical(self, K, lws, H, W, colors=True, **kw):
        """A CANONICAL-space snapshot: the canonical volume T ray-cast as it is stored, with NO warp field applied -- this is not
        a view of the live frame (that is render_live: the canonical mesh warped into the frame, K11).  Where the field is
        near the identity the two look alike; where it is not, this shows the reference pose.  K: the intrinsics to cast
        through (None: the frame's).  colors=True adds `.color` when the frame has a colour volume.  Single rank only: the ranks'
        slab casts would need a merge of their depth maps, which is not implemented (ValueError).  **kw goes to kernels.raycast."""
        if self.ws > 1:
            raise ValueError("raycast_canonical casts one rank's whole grid; the %d-rank slab partition is not supported" % self.ws)
        K = self.K if K is None else np.asarray(K, dtype=np.float64)
        lws = [lws] if np.asarray(lws[0]).ndim == 1 else list(lws)
        if colors and self.C is not None:
            kw.setdefault("colors", self.C)
            kw.setdefault("want", ("depth", "normals", "color"))
        R = self.R
        return kernels.raycast(self.T, self.Wt, K, np.linalg.inv(K), lws, H, W, self.scale, self.center, tsdf_res=R, res=(R, R, R),
                               x_range=(self.a, self.b), **kw)

    def colored_mesh(self, min_component_faces=None, simplify_cell=None, smooth_iters=None):
        """The canonical mesh with vertex colours: marching cubes of T at level 0 and the colour volume sampled at its vertices
        (kernels.sample_colors) -> (verts, faces, normals, rgb (n, 3) float32 in [0, 255], valid (n,) bool).  Single rank only, as
        render_live.  min_component_faces: drop the connected components with fewer faces (mesh.filter_components).  simplify_cell:
        then cluster the vertices at that cell size in voxels (mesh.simplify); the colours are sampled at the new vertices.
        smooth_iters: that many Taubin iterations (mesh.smooth_with_normals) after the component filter and before the
        simplification; the colours are sampled at the moved vertices."""
        if self.ws > 1:
            raise ValueError("colored_mesh extracts one rank's whole grid; the %d-rank slab partition is not supported" % self.ws)
        if self.C is None:
            raise ValueError("no colour volume: construct the frame with color_band")
        from . import mesh as _mesh
        verts, faces, normals, _ = _mesh.marching_cubes(self.T, 0.0, 1)
        if min_component_faces is not None:      # without the fragments: components with fewer faces are dropped first
            verts, faces, normals, _ = _mesh.filter_components(verts, faces, normals, min_faces=min_component_faces)
        if smooth_iters is not None:
            verts, normals = _mesh.smooth_with_normals(verts, faces, smooth_iters)
        if simplify_cell is not None:
            verts, faces, normals, _ = _mesh.simplify_with_normals(verts, faces, normals, simplify_cell)
        rgb, valid = kernels.sample_colors(self.C, verts.double())
        return verts, faces, normals, rgb, valid

    def _track(self, depth_list, lw_list):
        """step(track=True): the tracked cameras of this frame's maps, from the priors lw_list."""
        if self.tracker is None:
            raise ValueError("step(track=True) needs the constructor's tracker")
        if self.track_model == "live":
            def model(lws, K, H, W):
                r = self.raycast_live(lws, H, W, K=K, want=("depth", "normals"))
                return r.depth, r.normals
            gate = None
        else:
            def model(lws, K, H, W):
                depth, normals, _ = self.render_live(lws, H, W, K=K)
                return depth, normals
            gate = False
        lws, self.track_stats = self.tracker.track(depth_list, lw_list, model, gate_normals=gate)
        self.tracked_lw = lws
        return lws

    def visible_samples(self, lws, H, W, stride=1, max_samples=None):
        """The visible-surface samples of the loop's current live model in the views `lws`: render_live's mesh, warp and
        K / scale / center / half -- marching cubes of T at level 0, warped by the solver's node field, rasterised -- and, for every
        `stride`-th covered pixel of every `stride`-th row, the UNWARPED vertices and normals interpolated at the pixel
        (mesh.render_samples): the canonical point and normal of the surface a camera sees there, DynamicFusion's model-to-frame
        sample.  Returns (pos (S,3), nrm (S,3), pixel (S,)), view-major in pixel order.  Single rank only, as render_live."""
        if self.ws > 1:
            raise ValueError("visible_samples renders one rank's whole grid; the %d-rank slab partition is not supported" % self.ws)
        if not self.has_graph:
            raise ValueError("no deformation graph yet: call construct_graph() first")
        from . import mesh as _mesh
        verts, faces, normals, _ = _mesh.marching_cubes(self.T, 0.0, 1)
        sv = self.fs.solver
        warped = verts
        if verts.shape[0] > 0:
            nbr, _ = sample_knn(verts, sv.node_pos, sv.node_w, self.knn)
            warped, _ = warp_points(verts, normals, self.ident_lw, nbr=nbr, node_dq=sv.node_dq, node_pos=sv.node_pos,
                                    node_w=sv.node_w)
        return _mesh.render_samples(warped, faces, verts, normals, self.K, lws, H, W, scale=self.scale, center=self.center,
                                    half=self.R / 2, stride=stride, max_samples=max_samples)

    def set_sample_source(self, source, lws=None, size=None, stride=1, max_samples=None):
        """Where refresh_samples() -- and so the end of every step() -- takes the solve's samples from.  "band" (the default):
        every band voxel of the canonical slab (extract_surface_samples).  "visible": visible_samples(lws, size[0], size[1],
        stride, max_samples), the model rendered into the views `lws` of size = (H, W); step() then replaces views and size by
        each frame's own cameras and depth-map size, so the model as that frame updated and warped it is what the next frame's
        solve sees.  With a graph in place the samples are refreshed at once.  Graph construction and growth keep using the band
        samples whatever the source.  Single rank only for "visible"."""
        if source not in self.SAMPLE_SOURCES:
            raise ValueError("sample source must be one of %s, got %r" % (self.SAMPLE_SOURCES, source))
        stride = int(stride)
        if stride < 1:
            raise ValueError("stride must be >= 1, got %d" % stride)
        if source == "visible":
            if lws is None or size is None:
                raise ValueError("the visible sample source needs its views (lws) and their size (H, W)")
            if self.ws > 1:
                raise ValueError("the visible sample source renders one rank's whole grid; %d ranks are not supported" % self.ws)
            H, W = (int(x) for x in size)
            self._src_lws, self._src_size = lws, (H, W)
        self._src_stride = stride
        self._src_max = None if max_samples is None else int(max_samples)
        self.sample_source = source
        if self.has_graph:
            self.refresh_samples()

    def step(self, depth, lw_cam, gn_iters=10, rw=5.0, lm_abs=10.0, lm_rel=1e-2, max_dist=2.0, huber=0.5, stage_ms=None,
             update_graph=False, on_updated=None, data_views=None, relax=None, global_iters=None, global_lm=0.1, global_stride=None,
             data_term="depth", global_built=None, update="volume", update_weight="node_distance", graph_sampler="host",
             normal_gate=_KEEP, colors=None, track=False):
        """track: True = lw_cam is a prior and the constructor's tracker finds the frame's cameras first (see there); unset, the frame
        issues the calls it always did.
        colors: None, or one uint8 (H, W, 3) / (H, W, 4) image per depth map of this frame: right after the TSDF update of
        either `update` route, and before the warp field decays, they are averaged into `self.C` through the field the update used
        (kernels.integrate_color on this rank's slab, with the update's workspace and its stored node indices where the buffer
        has them) -- colour and geometry see the same field.  Needs the constructor's color_band.  The call reads T, Wt, the maps
        and the nodes and writes only `self.C`; without colours the frame issues the calls it always did.
        normal_gate: this call's normal gate (a cosine, or None for none) instead of the constructor's; see there.
        update: how the canonical slab takes the frame in.  "volume" = the reference's two stages: the live volume fused from
        the depth maps (K1) is resampled through the warp field (K3, kernels.fuse_volume_dqb; the warp gathers across slab faces,
        so several ranks all-gather the live volume).  "depth" = DynamicFusion's surface fusion (K1w,
        kernels.integrate_depth_dqb): every canonical voxel of this rank's slab is warped into the live frame, projected into the
        frame's depth maps and the projective signed distance averaged in with `update_weight` ("node_distance": K3's weights,
        so the canonical weights keep their meaning when a loop switches routes; "unit": K1's).  It reads no live volume: with
        data_term="depth" the frame then launches no live sweep and no all-gather and `self.live` is not written; with
        data_term="volume" the live volume is still swept (and gathered) for the solve only.
        data_term: "depth" = projective association against the depth maps (one projection and one pixel per sample and
        view; the live sweep overlaps the whole solve); "volume" = association against the live TSDF volume the frame fuses from
        all views anyway (FrameSolver.gn_iteration_volume: one trilinear cell per sample whatever the number of views, band =
        the truncation distance; the live sweep is joined -- and, on several ranks, all-gathered -- BEFORE the solve, and data_views
        does not apply).
        global_built: where the rigid-mode steps come from.  None keeps each term's choice: straight from the samples of every
        `global_stride`-th tile for "depth" (FrameSolver.global_iteration), from the built system for "volume", where
        global_stride then does not apply.  data_term="volume", global_built=False: from the samples, against the volume
        (FrameSolver.global_iteration_volume(built=False)), and global_stride applies.  For "depth" the argument is not read.
        Defaults (regulariser weight, LM damping, association gate and Huber threshold in voxels, the per-frame decay of the warp
        field `relax` = 0.8) are the ones under which the loop follows a +-0.6 voxel oscillation of the bench scene with a BOUNDED
        warp field: max node translation 0.85 voxel at frame 400, 1.01 at frame 1 200, sample count constant (tools/soak.py;
        tests/test_gpu_pipeline.py::test_soak_300_frames runs 300 of them).  Without the decay (relax = 1, round 3) nothing
        pulls a node back: 2.3 voxels at frame 400 and growing, the |T| < band shell thickens and the sample count doubles.  With
        a 4-voxel gate and weak damping, nodes without data support wander and the TSDF update corrupts the canonical volume.
        stage_ms: optional dict; when given, the device is synchronised after every stage and the stage's wall
        time (ms) is added under its name (for breakdowns only: the syncs cost throughput).
        on_updated: optional callable, called once the launches of this frame's TSDF update are queued and `self.updated` is
        recorded -- the place where a consumer of the updated canonical slab (mesh extraction on another stream) queues its
        first launches, ahead of the sample refresh's.
        graph_sampler: update_graph()'s `sampler` for update_graph=True."""
        if graph_sampler not in ("host", "device"):              # (graph.SAMPLERS; read by update_graph=True only)
            raise ValueError("graph_sampler must be 'host' or 'device', got %r" % (graph_sampler,))
        if data_term not in ("depth", "volume"):
            raise ValueError("data_term must be 'depth' or 'volume'")
        if update not in ("depth", "volume"):
            raise ValueError("update must be 'depth' or 'volume'")
        if update == "depth" and update_weight not in kernels.WARPED_WEIGHTS:
            raise ValueError("update_weight must be one of %s" % sorted(kernels.WARPED_WEIGHTS))
        gate_cos = self.normal_gate if normal_gate is SlabFrame._KEEP else self._check_normal_gate(normal_gate, self.depth_prep)
        if gate_cos is not None and data_term != "depth":
            raise ValueError("normal_gate is the depth data term's: data_term must be 'depth'")
        if colors is not None and self.color_band is None:
            raise ValueError("step(colors=...) needs the constructor's color_band: there is no colour volume")
        if not self.has_graph:
            raise ValueError("no deformation graph yet: call construct_graph() first")
        need_live = update == "volume" or data_term == "volume"       # (update="depth" fuses the maps themselves)
        import time as _t
        t0 = [_t.perf_counter()]

        def mark(name):
            if stage_ms is not None:
                torch.cuda.synchronize()
                now = _t.perf_counter()
                stage_ms[name] = stage_ms.get(name, 0.0) + (now - t0[0]) * 1e3
                t0[0] = now
        R = self.R
        # `depth` / `lw_cam` may be lists: the live volume is then fused from all of them (as the reference's
        # compute_live_tsdf does, core/fusion_dm.py:166-170) and the warp solve associates every sample against all of them
        # (the view in which it lies closest to the observed surface: dfh_gn_associate; data_views=1 keeps round 2's
        # first-view-only data term)
        depth_list = list(depth) if isinstance(depth, (list, tuple)) else [depth]
        lw_list = list(lw_cam) if isinstance(depth, (list, tuple)) else [lw_cam]
        if len(depth_list) != len(lw_list):
            raise ValueError('length of camera matrix array must equal that of depth maps')
        if colors is not None:
            colors = list(colors) if isinstance(colors, (list, tuple)) else [colors]
            if len(colors) != len(depth_list):
                raise ValueError('one colour image per depth map: %d images for %d maps' % (len(colors), len(depth_list)))
        color_depth_list = None
        if self.ingest is not None:               # raw frames in: everything below sees what it always saw
            depth_list, reg, color_depth_list = self._ingest(depth_list, colors)
            colors = reg if colors is not None else None
            mark("ingest")
        if self.depth_prep is not None:
            shape = (len(depth_list),) + tuple(depth_list[0].shape)
            if self._prep_out is None or tuple(self._prep_out[0].shape) != shape or self._prep_out[0].device != depth_list[0].device:
                dev = depth_list[0].device
                self._prep_out = (torch.empty(shape, dtype=torch.float32, device=dev),
                                  torch.empty(shape + (3,), dtype=torch.float32, device=dev))
            depth_list, self.live_normals = self.depth_prep(depth_list, self.Kinv, out=self._prep_out)
            self.clean_depth = depth_list
            mark("depth_prep")
        if track:
            lw_list = self._track(depth_list, lw_list)
            mark("track")
        depth, lw_cam = depth_list[0], lw_list[0]
        nd = len(depth_list) if data_views is None else max(1, min(int(data_views), len(depth_list)))
        solve_depth, solve_lw = (depth_list[:nd], lw_list[:nd]) if nd > 1 else (depth, lw_cam)
        gate_kw = {} if gate_cos is None else {"normals": self.live_normals[:nd], "normal_cos": gate_cos}
        def sweep_live():
            if self.ws_views is None:
                self.ws_views = kernels.integrate_workspace(min(len(depth_list), 16), depth.shape[0], depth.shape[1], (R, R, R), (self.a, self.b), self.live.device)
            kernels.integrate_depth_views(self.live, self.live_w, depth_list, self.K, self.Kinv, lw_list, self.scale, self.center,
                                          self.tdist_world, tsdf_res=R, res=(R, R, R), x_range=(self.a, self.b), workspace=self.ws_views,
                                          fresh=self.tvox)          # (the fill of the live volume is part of the sweep)
            self._live_views = (lw_list, int(depth.shape[0]), int(depth.shape[1]))
        # The solve reads the depth maps (projective association), not the live volume; the live volume depends on the depth maps
        # only and is first read by the TSDF update.  So the live-volume sweep (bandwidth-bound) runs on a side stream beside the
        # plan's launches AND the whole solve (bound by latency, ten waves per CU), and the streams join in front of the TSDF
        # update (round 4; rounds 2-3 joined before the first GN iteration).  With stage timing the order is sequential.
        joined = True
        if not need_live:
            pass
        elif stage_ms is None and not _lib.opt_on("py_no_side_stream"):
            if self._side is None:
                self._side = torch.cuda.Stream()
            main = torch.cuda.current_stream()
            self._side.wait_stream(main)             # the previous frame's TSDF update has read the live volume
            with torch.cuda.stream(self._side):
                sweep_live()
            self.fs.solver.prepare()
            joined = False
        else:
            sweep_live()
        mark("live_tsdf")
        # the rigid mode first (two steps: one twist shared by all nodes, fitted to the data rows -- FrameSolver.global_iteration),
        # then the node iterations (one host call: nothing between their launches depends on the host)
        ng = self.GLOBAL_ITERS if global_iters is None else int(global_iters)
        lm_on = self.fs.landmarks_active()     # (landmarks: the rigid-mode steps from the built system, which holds their rows)
        photo_kw = {}
        if colors is not None and self.photo_weight > 0.0 and data_term == "depth" and self.fs.photometric_active():
            photo_kw = {"colors": colors[:nd]}   # (the colour rows likewise: they are compared with the views the solve reads)
            lm_on = True
        live_full = None
        if data_term == "volume":
            # the solve reads the live volume: the side stream (which has overlapped the plan's launches) joins here, and the
            # whole volume is gathered now -- the TSDF update below reuses it
            if not joined:
                torch.cuda.current_stream().wait_stream(self._side)
                joined = True
            live_full = self.D.allgather_planes(self.live, R) if self.ws > 1 else self.live
            # band = the truncation distance AS STORED (the sweep's fresh value, rounded to the volume's type): the band test is
            # strict, so the cells that touch a voxel no view updated drop out
            band = float(torch.tensor(self.tvox, dtype=self.live.dtype))
            if ng > 0:
                sampled = global_built is not None and not global_built and not lm_on
                self.fs.global_iteration_volume(live_full, band, rw=rw, max_dist=max_dist, huber=huber, lm_rel=global_lm, n_iters=ng,
                                                built=not sampled, stride=self.GLOBAL_STRIDE if global_stride is None else int(global_stride))
            self.fs.gn_iteration_volume(live_full, band, rw=rw, lm_abs=lm_abs, lm_rel=lm_rel, max_dist=max_dist, huber=huber,
                                        n_iters=gn_iters)
        elif ng > 0 and not lm_on:
            # (every `global_stride`-th tile of THIS rank's samples: with the samples sharded over ranks a stride > 1 thins another
            # subsample than one GPU does -- the same estimator on other data; stride 1 is partition-independent)
            self.fs.global_iteration(solve_depth, solve_lw, max_dist=max_dist, huber=huber, lm_rel=global_lm, n_iters=ng,
                                     stride=self.GLOBAL_STRIDE if global_stride is None else int(global_stride), **gate_kw)
        if data_term == "depth":
            self.fs.gn_iteration(solve_depth, solve_lw, rw=rw, lm_abs=lm_abs, lm_rel=lm_rel, max_dist=max_dist, huber=huber, n_iters=gn_iters,
                                 n_global=ng if lm_on else 0, global_lm=global_lm, **gate_kw, **photo_kw)
        mark("solve")
        if not joined:
            torch.cuda.current_stream().wait_stream(self._side)
        if live_full is None and update == "volume":
            live_full = self.D.allgather_planes(self.live, R) if self.ws > 1 else self.live
        mark("allgather")
        sv = self.fs.solver
        if update == "volume":
            kernels.fuse_volume_dqb(self.T, self.Wt, live_full, sv.node_pos, sv.node_dq, sv.node_w, self.knn, self.ident_lw, self.tvox,
                                    res=(R, R, R), x_range=(self.a, self.b), workspace=self.ws_dqb, rebuild_candidates=self._first)
        else:
            kernels.integrate_depth_dqb(self.T, self.Wt, depth_list, self.K, self.Kinv, lw_list, self.scale, self.center,
                                        self.tdist_world, sv.node_pos, sv.node_dq, sv.node_w, self.knn, self.ident_lw,
                                        weight=update_weight, tsdf_res=R, res=(R, R, R), x_range=(self.a, self.b),
                                        workspace=self.ws_dqb, rebuild_candidates=self._first)
        self._first = False
        if colors is not None:                 # through the field the update used: before it decays
            # (with ingest: the maps that keep only the pixels with a valid colour -- the stage's own, unfiltered by depth_prep)
            kernels.integrate_color(self.C, self.T, self.Wt, depth_list if color_depth_list is None else color_depth_list, colors,
                                    self.K, self.Kinv, lw_list, self.scale, self.center,
                                    self.tdist_world, self.color_band, sv.node_pos, sv.node_dq, sv.node_w, self.knn, self.ident_lw,
                                    tsdf_res=R, res=(R, R, R), x_range=(self.a, self.b), workspace=self.ws_dqb,
                                    stored_indices=kernels.dqb_has_indices(self.ws_dqb, (R, R, R), self.knn, int(sv.node_pos.shape[0]),
                                                                           (self.a, self.b)))
        # the warp field decays towards the identity once the TSDF update has used it (solve.relax_twists: every node's rotation
        # vector and translation scaled by `relax`).  Fusion.updateTSDF writes most of the motion into the canonical volume every
        # frame, and without a term that pulls a node back the field random-walks over hundreds of frames
        # (tools/soak.py; tests/test_gpu_pipeline.py::test_soak_300_frames).  relax = 1 keeps round 3's behaviour.
        rx = self.RELAX if relax is None else float(relax)
        if rx != 1.0:
            relax_twists(sv.node_dq, rx)
        if self.updated is None:
            self.updated = torch.cuda.Event()
        self.updated.record()                  # the canonical slab of this frame is final from here on (a consumer on another
        if on_updated is not None:             # stream, e.g. mesh extraction, need not wait for the sample refresh below)
            on_updated()
        mark("tsdf_update")
        if self.sample_source == "visible":              # this frame's cameras and map size: the prediction for the next frame
            self._src_lws, self._src_size = lw_list, (int(depth.shape[0]), int(depth.shape[1]))
        self.photo_active = sv._ph["active"] if photo_kw and sv._ph is not None else None      # (the refresh replaces the term's arrays)
        n = self.refresh_samples()
        mark("samples")
        self.fs.solver.check_status(completed_only=True)   # the sample count's read-back has synchronised: a timed-out PCG raises here
        if update_graph:
            if self.update_graph(sampler=graph_sampler):
                n = self.fs.solver.S
                self._refresh_photo()              # (a new graph dropped the term with its plan)
            mark("graph")
        return n
