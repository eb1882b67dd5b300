"""`FusionDM` with the reference's call surface (reference core/fusion_dm.py:53-354),
running its per-voxel hot methods as HIP kernels on an MI355X.

The reference's own device plug-in is a subclass overriding one numpy-in / numpy-out
method (class FusionDM_GPU, core/fusion_dm.py:563-574,600); this class keeps the same
method names, argument order, in-place + return ownership and ValueError behaviour, so
`FusionDM(tdist, K, tsdf_res=...)` / `.fuseDepths(...)` / `.compute_live_tsdf(...)` /
`.updateTSDF(...)` / `.computef_lw(...)` / `.solve(...)` call sites keep working.

What differs, on purpose:
  * volumes live on the GPU as float32 (16 B/voxel read-modify-write; pass
    `volume_dtype=np.float64` for bit-for-bit float64 volumes).  `_tsdf` / `_tsdfw` are
    properties that download on read and upload on assignment;
  * methods accept CUDA tensors wherever the reference takes numpy arrays, and then work
    in place without host round trips;
  * semantics are the reference's CPU path (fuseDepths :180-217), not its OpenCL kernel
    (:600-737), which computes something else;
  * no CPU fallback: without the HIP library / a GPU the hot methods raise.
"""
import os

import numpy as np
import torch
from numpy import linalg as la

from . import kernels, mesh as _mesh, solve as _solve
from .canonical import CanonicalModel, _is_tensor
from .device import depths_to_device, require_gpu, to_device


class FusionDM(CanonicalModel):
    _mc_level = 0.0              # write_canonical_mesh / live_frame_mesh extract the zero level set (core/fusion_dm.py:341)
    _live_tensor_error = 'Only accept 3D array as tsdf'
    _weight_arg = 'tsdf_w'
    _unit_weight_samples = False  # surface_samples gates on the fused weights as they are (Fusion: see there)

    def __init__(self, trunc_distance, K, tsdf_res=256, subsample_rate=5.0, knn=4, marching_cubes_step_size=3,
                 verbose=False, write_warpfield=True, volume_dtype=np.float32):
        # attribute set of the reference ctor, core/fusion_dm.py:57-81
        self._init_model(trunc_distance, subsample_rate, knn, marching_cubes_step_size, verbose, write_warpfield, volume_dtype)
        self._tsdf_res = tsdf_res
        self._lw = np.array([1, 0, 0, 0, 0, 0, 0, 0], dtype=np.float32)

        K = np.asarray(K, dtype=np.float64)
        if K.shape != (3, 3):
            raise ValueError('intrinsic matrix K must be 3x3')
        self._K = K
        self._Kinv = la.inv(K)

        self._IND = np.eye(4)
        self._INDinv = la.inv(self._IND)
        self._corridx = []

    def verbose_gpu(self):
        """What the reference's device plug-in prints about its OpenCL devices (FusionDM_GPU.verbose_gpu, core/fusion_dm.py:576-598),
        for the HIP devices this process sees: name, compute units, clock, memory, LDS and workgroup limits, the library's ABI."""
        from . import _lib
        print('\n' + '=' * 60 + '\nHIP devices (libdfusion_hip ABI %d)' % _lib.ABI_VERSION)
        if not torch.cuda.is_available():
            print('    none visible')
        for i in range(torch.cuda.device_count()):
            p = torch.cuda.get_device_properties(i)
            print('=' * 60)
            print('    Device %d - Name:  %s (%s)' % (i, p.name, getattr(p, "gcnArchName", "")))
            print('    Device - Compute Units:  {0}'.format(p.multi_processor_count))
            print('    Device - Max Clock Speed:  {0:.0f} Mhz'.format(getattr(p, "clock_rate", 0) / 1e3))
            print('    Device - Local Memory:  {0:.0f} KB'.format(getattr(p, "shared_memory_per_block", 0) / 1024.0))
            print('    Device - Global Memory: {0:.0f} GB'.format(p.total_memory / 1073741824.0))
            print('    Device - Max Work Group Size: {0:.0f}'.format(getattr(p, "max_threads_per_block", 1024)))
        print('\n')

    # ------------------------------------------------------------------ volumes
    def _new_volume_pair(self, res=None):
        require_gpu()
        r = self._tsdf_res if res is None else res
        shape = (r, r, r) if np.isscalar(r) else tuple(r)
        T = torch.full(shape, self._tdist, dtype=self._vol_dtype, device="cuda")      # :61 / :100
        Wt = torch.zeros(shape, dtype=self._vol_dtype, device="cuda")                 # :62 / :101
        return T, Wt

    def _ensure_volumes(self):
        if self._T is None or self._Wt is None:
            T, Wt = self._new_volume_pair()
            self._T = T if self._T is None else self._T
            self._Wt = Wt if self._Wt is None else self._Wt

    # ------------------------------------------------------------------ A1
    def _depth_to_device(self, dm):
        if _is_tensor(dm):
            if dm.dim() != 2:
                raise ValueError('depth map must be 2-D')
            d = dm if dm.dtype in (torch.float32, torch.float64) else dm.to(torch.float32)
            return to_device(d)
        dm = np.asarray(dm)
        if dm.ndim != 2:
            raise ValueError('depth map must be 2-D')
        return depths_to_device([dm])[0]        # float32 on device unless that would change a value (then masks could flip)

    def fuseDepths_ocl(self, dm, lw, tsdf, tsdf_w, wmax=100.0):
        """The reference's OTHER fuseDepths: FusionDM_GPU's OpenCL kernel (core/fusion_dm.py:600-737), whose arithmetic differs
        from the CPU path (float32 throughout, bilinear depth, index -> pixel through `_IND`, pixels
        without depth carve free space, opposite sign, no `scale`).  Like the reference's host code it leaves its inputs alone
        and returns NEW float32 arrays (:690-691,:737); CUDA tensors in, CUDA tensors out."""
        lw = np.asarray(lw, dtype=np.float64)
        if lw.shape != (3, 4):
            raise ValueError('lw must be a 3x4 camera extrinsic')
        if _is_tensor(tsdf) != _is_tensor(tsdf_w):
            raise ValueError('tsdf and tsdf_w must both be numpy arrays or both CUDA tensors')
        proj = np.matmul(self._K, np.matmul(lw, self._IND)).astype(np.float32)             # :695
        kinv = self._Kinv.astype(np.float32)                                                # :697
        tdist_lit = np.float32(float("%f" % self._tdist))                                   # "#define TDIST %ff" (:682-687)
        wmax_lit = np.float32(float("%f" % wmax))
        depth = to_device(dm if _is_tensor(dm) else np.asarray(dm), dtype=torch.float32)    # dm.astype(np.float32), :698
        if depth.dim() != 2:
            raise ValueError('depth map must be 2-D')
        if _is_tensor(tsdf):
            T, Wt = tsdf.to(dtype=torch.float32).clone().contiguous(), tsdf_w.to(dtype=torch.float32).clone().contiguous()
        else:
            if tsdf.ndim != 3 or tsdf.shape != tsdf_w.shape:
                raise ValueError('tsdf and tsdf_w must be 3-D arrays of the same shape')
            T, Wt = to_device(tsdf.astype(np.float32)), to_device(tsdf_w.astype(np.float32))   # :690-691
        kernels.integrate_depth_ocl(T, Wt, depth, proj, kinv[2], tdist_lit, wmax_lit)
        if _is_tensor(tsdf):
            return (T, Wt)
        return (T.cpu().numpy(), Wt.cpu().numpy())

    def fuseDepths(self, dm, lw, tsdf, tsdf_w, scale=1.0, center=np.zeros(3), wmax=100.0, mode="cpu"):
        """Integrate one depth map into (tsdf, tsdf_w); reference core/fusion_dm.py:180-217.

        numpy volumes are updated in place AND returned (the reference mutates through
        np.nditer and returns the same arrays, :186,:217); CUDA tensors are updated in place
        with no host traffic.  mode="ocl": the arithmetic of the reference's OpenCL override instead
        (fuseDepths_ocl: new float32 arrays, `scale` / `center` unused as there)."""
        if mode == "ocl":
            return self.fuseDepths_ocl(dm, lw, tsdf, tsdf_w, wmax)
        if mode != "cpu":
            raise ValueError('mode must be "cpu" (FusionDM.fuseDepths semantics) or "ocl" (FusionDM_GPU.fuseDepths semantics)')
        lw = np.asarray(lw, dtype=np.float64)
        if lw.shape != (3, 4):
            raise ValueError('lw must be a 3x4 camera extrinsic')
        return self._fuse_depth_into(self._depth_to_device(dm), lw, tsdf, tsdf_w, scale, center, wmax, self._tsdf_res)

    # ------------------------------------------------------------------ A3
    def updateTSDF(self, curr_tsdf, wmax=100.0):
        """Rigidly warp every canonical voxel by `_lw` into the live TSDF, sample it and fuse;
        reference core/fusion_dm.py:300-316.  Mutates `_tsdf` / `_tsdfw` (on the GPU)."""
        live = self._live_to_device(curr_tsdf)
        self._ensure_volumes()
        kernels.fuse_volume_rigid(self._T, self._Wt, live, np.asarray(self._lw, dtype=np.float64), self._tdist, wmax)

    # ------------------------------------------------------------------ A9
    def _corr_state(self):
        if self._vertices is None or self._normals is None:
            raise ValueError('canonical vertices / normals have not been set')
        idx = np.asarray(self._corridx, dtype=np.int64)
        C = np.asarray(self._correspondences, dtype=np.float64).reshape(-1, 3)
        if len(idx) != len(C):
            raise ValueError('_corridx and _correspondences disagree in length')
        V = np.asarray(self._vertices, dtype=np.float64)[idx]
        Nn = np.asarray(self._normals, dtype=np.float64)[idx]
        return V, Nn, C

    def computef_lw(self, x):
        """Point-to-plane residual of the kept correspondences under the global transform x;
        reference core/fusion_dm.py:285-297."""
        V, Nn, C = self._corr_state()
        return _solve.residual_rigid(x, V, Nn, C).cpu().numpy()

    # ------------------------------------------------------------------ surface + correspondences
    def marching_cubes(self, tsdf=None, step_size=1):
        """Mesh vertices / faces / normals of the level set; reference core/fusion_dm.py:319-331
        (`measure.marching_cubes_lewiner(volume, step_size=step_size)`: no level is passed, so skimage's
        default (min + max) / 2 applies -- reproduced).  With `tsdf` returns (verts, faces, normals,
        values) as numpy arrays; without, fills `_vertices` / `_faces` / `_normals` from the canonical
        volume.  Runs on the GPU (csrc/dfh_mesh.hip); conventions and what is pinned: mesh.py."""
        return self._marching_cubes(tsdf, step_size)

    def render_model(self, lws, H, W, K=None, scale=1.0, center=np.zeros(3), **kw):
        """KinectFusion's surface prediction (not in the reference): the canonical volume ray-cast into the views `lws` (one 3x4
        world->camera matrix or a list), voxels mapped to world by K1's rule (scale, center, half = tsdf_res / 2) -- pass the
        scale and center the volume was fused with.  K defaults to `_K`.  Returns kernels.raycast's result (.depth in the maps'
        convention, .normals, and .color when there is a colour volume `_C`); **kw goes to kernels.raycast (step, min_weight,
        refine, z_near, z_far, want, table, ...).  No mesh is built."""
        K = self._K if K is None else np.asarray(K, dtype=np.float64)
        return self._raycast_canonical(lws, H, W, K, scale, center, self._tsdf_res, **kw)

    def track_frame(self, depths, lws_prev, tracker, scale=1.0, center=np.zeros(3), **kw):
        """KinectFusion's pose estimation (not in the reference): the cameras of the depth maps `depths`, found by the
        tracking.CameraTracker `tracker` from the priors `lws_prev` (one 3x4 world->camera matrix per map) against the canonical
        volume, ray-cast by render_model into the prior cameras at every pyramid level's K (scale, center: the ones the volume
        was fused with; **kw goes to the ray cast).  Returns CameraTracker.track's (lws, stats); nothing of the object changes."""
        def model(lws, K, H, W):
            r = self.render_model(lws, H, W, K=K, scale=scale, center=center, want=("depth", "normals"), **kw)
            return r.depth, r.normals
        return tracker.track(depths, lws_prev, model)

    def _write_mesh(self, fpath, verts, faces, normals, colors=None, valid=None):
        """World coordinates through `_IND`, `v` / `vn` / `f a//a b//b c//c` (core/fusion_dm.py:339-354)."""
        _mesh.write_obj(fpath, verts, faces, normals, ind=self._IND, colors=colors, valid=valid)

    def average_edge_dist_in_face(self, f):
        """Reference core/fusion_dm.py:360-364.  (Not shared with Fusion: this one measures in the vertices' own dtype, that one
        in float64, and the results differ in the last bits.)"""
        v1, v2, v3 = (np.asarray(self._vertices[i]) for i in f[:3])
        d = lambda a, b: np.linalg.norm(a - b)
        return (d(v1, v2) + d(v1, v3) + d(v2, v3)) / 3

    def setupCorrespondences(self, curr_tsdf, prune_result=True, tolerance=1.0, live_vertices=None):
        """Closest-point correspondences of the canonical vertices in the live surface; reference
        core/fusion_dm.py:219-244 (warp by `_lw`, knn nearest live vertices, smallest point-to-plane
        cost, keep if <= tolerance).  `live_vertices` replaces the marching-cubes call on curr_tsdf."""
        if self._vertices is None or self._normals is None:
            raise ValueError('canonical vertices / normals have not been set (call marching_cubes())')
        lverts = self.marching_cubes(curr_tsdf, step_size=1)[0] if live_vertices is None else np.asarray(live_vertices, dtype=np.float64)
        if len(lverts) < self._knn:
            raise ValueError('fewer live vertices than knn')
        lw = np.asarray(self._lw, dtype=np.float64)
        vp, wn = _solve.warp_points(self._vertices, self._normals, lw)
        corr, cost, keep = _solve.closest_correspondences(vp, wn, lverts, self._knn, tolerance)
        keep = keep.cpu().numpy().astype(bool)
        self._corridx = list(np.nonzero(keep)[0])
        self._correspondences = list(corr.cpu().numpy()[keep])

    def solve(self, curr_tsdf=None, iterations=10):
        """Rigid alignment `_lw`; call surface of reference core/fusion_dm.py:264-282: three rounds
        of [setupCorrespondences(curr_tsdf) -> minimise 0.5*|computef_lw|^2 from the current `_lw`].
        The reference minimises with scipy's least_squares (finite differences); here Gauss-Newton
        on the 6-DoF left twist with analytic Jacobians (HIP kernels).  curr_tsdf=None keeps the
        correspondences already stored in `_corridx` / `_correspondences` (one round)."""
        self._itercounter += 1
        self.last_costs = []
        for _ in range(3 if curr_tsdf is not None else 1):             # iteration = 3, :265
            if curr_tsdf is not None:
                self.setupCorrespondences(curr_tsdf)
            V, Nn, C = self._corr_state()
            x, costs = _solve.solve_rigid_gn(np.asarray(self._lw, dtype=np.float64), V, Nn, C, iters=iterations)
            self._lw = x
            self.last_costs.append(costs)

    # ------------------------------------------------------------------ driver
    def _auto_alignment(self, depths, lws):
        """Centre / spread of the back-projected depth pixels (intent of
        core/fusion_dm.py:110-134; that loop cannot run for more than one view at HEAD
        because `avgs` is turned into an ndarray inside it, :131)."""
        avgs, stds = [], []
        for dm, A in zip(depths, lws):
            dm = dm.cpu().numpy() if _is_tensor(dm) else np.asarray(dm)
            A = np.asarray(A, dtype=np.float64)
            rows, cols = np.nonzero(dm)
            uv = -1 * dm[rows, cols][:, None] * np.stack([cols, rows, np.ones_like(rows)], axis=1).astype(float)
            pos3 = uv @ self._Kinv.T
            Rinv = la.inv(A[:, :3])
            pts = (pos3 - A[:, 3]) @ Rinv.T
            avgs.append(np.average(pts, axis=0))
            stds.append(np.std(pts, axis=0))
        return np.average(np.array(avgs), axis=0), float(np.average(np.array(stds)))

    def compute_live_tsdf(self, depths, lws, UseAutoAlignment=False, useICP=False, outputMesh=False,
                          as_numpy=True, mesh_path='.', colors=None, color_band=1.5):
        """Fuse a set of depth maps into a fresh volume; reference core/fusion_dm.py:95-178.
        The volume stays on the GPU across views; `as_numpy=False` returns the CUDA
        tensors instead of downloading them.
        colors (not in the reference): one uint8 (H, W, 3) / (H, W, 4) image per depth map; after the sweep they are averaged
        into a fresh colour volume `_C` (kernels.integrate_color, no warp) on the voxels within color_band voxels of the surface,
        and write_canonical_mesh writes vertex colours.  Without colours `_C` is None."""
        if len(depths) != len(lws):
            raise ValueError('length of camera matrix array Ks must equal that of depth maps')   # :96-97
        if colors is not None:
            if useICP:
                raise ValueError('colors cannot be fused with useICP=True: every view gets a rigid alignment of its own there')
            if len(colors) != len(depths):
                raise ValueError('one colour image per depth map')
        depths, colors, color_depths = self._prepare_depths(depths, colors)   # (the single-map fuseDepths stays raw)
        avg = np.array([-0.03, -0.43, -5.6], dtype='float32')       # :106-107
        std = 1.3
        if UseAutoAlignment:
            avg, std = self._auto_alignment(depths, lws)

        res = self._tsdf_res
        scale = 8 * std / res                                       # :136-141
        self._IND[0, 0] = scale
        self._IND[1, 1] = scale
        self._IND[2, 2] = scale
        self._IND[0:3, 3] = avg - scale * res / 2
        self._INDinv = la.inv(self._IND)

        if useICP:                                                  # :149-164
            for idx in range(len(depths)):
                T, Wt = self._new_volume_pair()
                self.fuseDepths(depths[idx], lws[idx], T, Wt, scale=10 * std / res, center=avg)
                if idx == 0:
                    self._T, self._Wt = T, Wt
                    self.marching_cubes()
                else:
                    self._lw = np.array([1, 0, 0, 0, 0, 0, 0, 0], dtype=np.float32)
                    self.solve(T)
                    self.updateTSDF(T)
            T, Wt = self._T, self._Wt
        else:
            dev = [self._depth_to_device(d) for d in depths]
            if len(dev) > 1 and len({(tuple(d.shape), d.dtype) for d in dev}) == 1 and \
                    all(np.asarray(l).shape == (3, 4) for l in lws):
                # the loop below as ONE sweep of the volume, the initial values (:100-101) included (same bits:
                # kernels.integrate_depth_views with fresh=)
                r = self._tsdf_res
                T = torch.empty((r, r, r), dtype=self._vol_dtype, device="cuda")
                Wt = torch.empty_like(T)
                kernels.integrate_depth_views(T, Wt, dev, self._K, self._Kinv, [np.asarray(l, dtype=np.float64) for l in lws],
                                              12 * std / res, avg, self._tdist, 100.0, tsdf_res=self._tsdf_res, fresh=self._tdist)
                self._depthidx = len(depths) - 1
            else:
                T, Wt = self._new_volume_pair()
                for idx in range(len(depths)):                      # :166-170
                    self._depthidx = idx
                    self.fuseDepths(dev[idx], lws[idx], T, Wt, scale=12 * std / res, center=avg)
            self._T, self._Wt = T, Wt
        self._C = None
        if colors is not None:
            self._C = kernels.color_volume(tuple(self._T.shape))
            for idx in range(len(dev)):                             # (one call per view: the maps may differ in shape or dtype)
                kernels.integrate_color(self._C, self._T, self._Wt, [dev[idx] if color_depths is None else color_depths[idx]],
                                        [colors[idx]], self._K, self._Kinv,
                                        [np.asarray(lws[idx], dtype=np.float64)], 12 * std / res, avg, self._tdist, color_band,
                                        tsdf_res=self._tsdf_res)
        if outputMesh:                                              # :174-176
            np.save(os.path.join(mesh_path, 'tsdf_temp'), self._T.cpu().numpy())     # the reference's `np.save('tsdf_temp', self._tsdf)` (:175), in mesh_path
            self.write_canonical_mesh(mesh_path, 'test.obj')
        if as_numpy:
            return (self._tsdf, self._tsdfw)
        return (T, Wt)
