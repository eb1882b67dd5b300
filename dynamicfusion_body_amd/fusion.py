"""`Fusion` (non-rigid DynamicFusion) with the reference's call surface
(reference core/fusion.py:49-598), its per-voxel / per-vertex hot methods running as HIP
kernels on an MI355X.

The reference constructor cannot run at HEAD (it reads an undefined `tsdf`,
core/fusion.py:51); callers pass the canonical TSDF first (test.py:74,110), which is the
signature kept here.  Marching cubes, correspondence search and graph maintenance are not
on this hot path: the deformation graph is supplied as the reference's own
`_nodes` list of 4-tuples (vertex index, position, dual quaternion, weight = 2*radius,
core/fusion.py:107-116), and `_vertices/_normals/_correspondences/_neighbor_look_up` are
plain arrays the caller fills.
"""
import numpy as np
import torch

from . import graph as _graph, kernels, mesh as _mesh, solve as _solve
from .canonical import CanonicalModel, _is_tensor
from .device import depths_to_device, require_gpu, to_device


class Fusion(CanonicalModel):
    _mc_level = None             # write_canonical_mesh / live_frame_mesh extract at skimage's default level, (min + max) / 2
    _live_tensor_error = 'Only accept 3D np array as tsdf'
    _weight_arg = 'tsdfw'
    # The constructor takes a finished TSDF and gives it zero weights (core/fusion.py:74): until something is fused, a weight gate
    # would leave surface_samples() nothing, so a never-fused volume is read with unit weights.  (FusionDM's volume only ever
    # comes out of a fusion; its zero weights mean "not observed" and stay a gate.)
    _unit_weight_samples = True
    descriptor_fn = None         # a callable (vertices (n,3), faces (m,3) or None) -> (n, D) float32 per-vertex descriptors: stands where
                                 # the reference calls compute_correspondence(self.input, self._feature, self._sess, vertices, faces)
                                 # (core/fusion.py:280-281); with it setupCorrespondences(method='cnn') takes the reference's CNN branch
                                 # (descriptors.PooledDescriptors(feature_fn) is that function around a per-pixel feature network)

    def __init__(self, tsdf, trunc_distance, subsample_rate=5.0, knn=4, marching_cubes_step_size=3, verbose=False,
                 use_cnn=False, write_warpfield=True, volume_dtype=np.float32):
        if not _is_tensor(tsdf) and (type(tsdf) is not np.ndarray or tsdf.ndim != 3):
            raise ValueError('Only 3D numpy array is accepted as tsdf')          # core/fusion.py:51-52
        if _is_tensor(tsdf) and tsdf.dim() != 3:
            raise ValueError('Only 3D numpy array is accepted as tsdf')
        if use_cnn:
            raise NotImplementedError('the CNN correspondence branch (core/sdf.py:75-150) is outside this hot path')
        self._init_model(trunc_distance, subsample_rate, knn, marching_cubes_step_size, verbose, write_warpfield, volume_dtype)
        self._lw = np.array([1, 0, 0, 0, 0, 0.1, 0, 0], dtype=np.float32)        # :57
        self.landmark_weight = 0.0               # > 0: solve() also uses the correspondences as POINTS (WarpSolver.set_landmarks)
        self._sess = None
        self._tsdf_host = tsdf                   # uploaded on first use (ctor works without a GPU)
        self._workspace = None
        self._workspace_key = None

    # ------------------------------------------------------------------ volumes
    def _ensure_volumes(self):
        if self._T is None:
            require_gpu()
            self._T = to_device(self._tsdf_host, dtype=self._vol_dtype)
            self._tsdf_host = None
        if self._Wt is None:
            self._Wt = torch.zeros_like(self._T)                                 # InitializeCanonicalSpace, :74

    @CanonicalModel._tsdf.setter
    def _tsdf(self, value):
        CanonicalModel._tsdf.fset(self, value)
        self._tsdf_host = None                   # the constructor's volume is superseded: it must not be uploaded later

    def volume_from_mesh(self, verts, faces, band=None, orientation=+1):
        """The signed-distance volume of a mesh given in the canonical volume's index coordinates (origin 0, spacing 1), with
        the canonical volume's shape and dtype: the exact distance inside `band` (default: the truncation distance), +-band
        beyond it (mesh.MeshDistance.grid).  The result goes straight into setupCorrespondences / updateTSDF."""
        from . import mesh
        self._ensure_volumes()
        band = self._tdist if band is None else float(band)
        md = mesh.MeshDistance(verts, faces, orientation=orientation, device=self._T.device)
        return md.grid(0.0, 1.0, tuple(self._T.shape), band, dtype=self._vol_dtype)

    # ------------------------------------------------------------------ A4
    def _dqb_workspace_for(self, pos, w, res):
        """(workspace, rebuild): the DQB workspace of updateTSDF / updateTSDF_depths (one serves both) and whether its stored
        candidates have to be recomputed -- they depend on the grid, the nodes' positions and weights, and knn."""
        key = (res, pos.tobytes(), w.tobytes(), self._knn)
        rebuild = key != self._workspace_key
        if rebuild:
            self._workspace = kernels.dqb_workspace(res, knn=self._knn, n_nodes=len(pos))
            self._workspace_key = key
        return self._workspace, rebuild

    def updateTSDF(self, curr_tsdf=None, wmax=100.0):
        """Warp every canonical voxel through the DQB warp field and `_lw` into the live TSDF,
        sample and fuse; reference core/fusion.py:153-198 (the debug prints :192-195 are not
        reproduced)."""
        if curr_tsdf is not None:
            self._curr_tsdf = curr_tsdf
        if self._curr_tsdf is None:
            raise ValueError('tsdf of live frame has not been loaded')           # :158-159
        live = self._live_to_device(self._curr_tsdf)
        self._ensure_volumes()
        pos, dq, w, _ = self.node_arrays()
        workspace, rebuild = self._dqb_workspace_for(pos, w, tuple(self._T.shape))
        kernels.fuse_volume_dqb(self._T, self._Wt, live, pos, dq, w, self._knn,
                                np.asarray(self._lw, dtype=np.float64), self._tdist, wmax,
                                workspace=workspace, rebuild_candidates=rebuild)

    def updateTSDF_depths(self, depths, lws, wmax=100.0, weight="node_distance", scale=1.0, center=np.zeros(3), colors=None,
                          color_band=1.5):
        """The canonical update straight from the frame's depth maps (K1w, dfh_integrate_depth_dqb): every canonical voxel is
        warped through the DQB warp field and `_lw` as in updateTSDF, projected into each map as in fuseDepths, and the
        projective signed distance is averaged in -- DynamicFusion's surface fusion, without the live volume updateTSDF
        resamples.  Needs the intrinsics of InitializeCanonicalSpace(..., K=K); depth maps follow fuseDepths' dtype rule
        (float32 on the device unless a float64 map is not float32-exact: then every map travels as float64).
        weight: "node_distance" = updateTSDF's running average (core/fusion.py:180-190), "unit" = fuseDepths'.
        colors: one uint8 (H, W, 3) / (H, W, 4) image per depth map; after the update they are averaged into the colour volume
        `_C` (kernels.integrate_color: the same nodes, `_lw` and workspace) on the voxels within color_band voxels of the
        canonical surface, and write_canonical_mesh writes vertex colours."""
        if getattr(self, '_K', None) is None:
            raise ValueError('updateTSDF_depths needs the intrinsics: call InitializeCanonicalSpace(..., K=K) first')
        depths, lws = list(depths), list(lws)
        if len(depths) != len(lws):
            raise ValueError('length of camera matrix array must equal that of depth maps')
        if weight not in kernels.WARPED_WEIGHTS:
            raise ValueError("weight must be one of %s, not %r" % (sorted(kernels.WARPED_WEIGHTS), weight))
        if colors is not None and len(colors) != len(depths):
            raise ValueError('one colour image per depth map')
        lws = [np.asarray(m, dtype=np.float64) for m in lws]
        for m in lws:
            if m.shape != (3, 4):
                raise ValueError('lw must be a 3x4 camera extrinsic')
        for d in depths:
            if (d.dim() if _is_tensor(d) else np.asarray(d).ndim) != 2:
                raise ValueError('depth map must be 2-D')
            if tuple(d.shape) != tuple(depths[0].shape):
                raise ValueError('all depth maps of one call must have the same shape')
        depths, colors, color_depths = self._prepare_depths(depths, colors)
        ds = depths_to_device(depths)
        self._ensure_volumes()
        pos, dq, w, _ = self.node_arrays()
        res = tuple(self._T.shape)
        workspace, rebuild = self._dqb_workspace_for(pos, w, res)
        kernels.integrate_depth_dqb(self._T, self._Wt, ds, self._K, self._Kinv, lws, scale, center, self._tdist, pos, dq, w,
                                    self._knn, np.asarray(self._lw, dtype=np.float64), wmax=wmax, weight=weight,
                                    tsdf_res=res[0], workspace=workspace, rebuild_candidates=rebuild)
        if colors is not None:
            if self._C is None:
                self._C = kernels.color_volume(res)
            kernels.integrate_color(self._C, self._T, self._Wt, ds if color_depths is None else color_depths, colors, self._K,
                                    self._Kinv, lws, scale, center, self._tdist, color_band, pos, dq, w, self._knn, np.asarray(self._lw, dtype=np.float64), tsdf_res=res[0],
                                    workspace=workspace, stored_indices=kernels.dqb_has_indices(workspace, res, self._knn, len(pos)))

    def computef_lw(self, x, tdw, trw):
        """Data rows with the global transform `x` in place of `_lw`; reference core/fusion.py:444-456."""
        V, Nn, nbr, C = self._vertex_state()
        pos, dq, w, _ = self.node_arrays()
        return _solve.residual_data(dq, V, Nn, C, nbr, pos, w, x).cpu().numpy()

    def setupCorrespondences(self, curr_tsdf, method='cnn', prune_result=True, tolerance=0.2, live_vertices=None, descriptors=None):
        """Closest-point correspondences of the DQB-warped canonical vertices in the live surface; reference
        core/fusion.py:243-314, the branch taken without a CNN session (`self._sess is None or method ==
        'clpts'`): live mesh by marching cubes, warp each vertex / normal with its blended node DQs and `_lw`,
        knn nearest live vertices, smallest point-to-plane cost.  With `prune_result`, vertices whose best cost
        exceeds `tolerance` are removed from `_vertices / _normals / _neighbor_look_up / _correspondences`, `_faces`
        is dropped and the nodes are re-anchored to their nearest remaining vertex (:297-313).  Not reproduced: at
        HEAD the pruned index is shadowed by the inner loop variable (`idx_pruned.append(idx)` appends a LIVE vertex
        index, :273-274) -- the intended canonical index is used.  `live_vertices` replaces the marching-cubes call.
        method='sdf' (not in the reference): the correspondences come straight from the live VOLUME (WarpSolver.associate_volume,
        band = the truncation distance, no gate; the volume holds distances in voxels) and `keep` is the association's validity;
        the pruning bookkeeping is the same.
        method='cnn' with `descriptors` = (s_feats (V, D), l_feats (L, D)) or with `descriptor_fn` set (the pair wins): the
        reference's CNN branch (:277-296).  Every canonical vertex takes the live vertex with the nearest descriptor
        (solve.nearest_descriptors: exact fp64 distances, lowest index on ties); with `prune_result` the vertices whose warped
        point-to-plane cost |n'.(v' - c)| exceeds `tolerance` are pruned (:288-296), and so is a vertex no live descriptor is
        comparable with (index -1: NaNs); without pruning such a vertex keeps its own warped position (a zero data row).  The
        live mesh is marching_cubes(curr_tsdf, step_size=1); with an explicit pair `live_vertices` may replace it.  Without a
        pair and without `descriptor_fn`, method='cnn' is the closest-points branch, as in the reference without a session."""
        if self._vertices is None or self._normals is None or len(self._neighbor_look_up) == 0:
            raise ValueError('canonical vertices / normals / _neighbor_look_up have not been set')
        self._curr_tsdf = curr_tsdf
        V = np.asarray(self._vertices, dtype=np.float64)
        Nn = np.asarray(self._normals, dtype=np.float64)
        nbr = np.asarray(self._neighbor_look_up, dtype=np.int64)
        pos, dq, w, _ = self.node_arrays()
        by_descriptor = method == 'cnn' and (descriptors is not None or self.descriptor_fn is not None)
        if by_descriptor and descriptors is not None:
            # shapes first: nothing below may touch the device with a pair that cannot be used
            if len(descriptors) != 2:
                raise ValueError('descriptors must be a pair (s_feats, l_feats)')
            _solve.check_descriptor_pair(descriptors[0], descriptors[1])
            if descriptors[0].shape[0] != len(V):
                raise ValueError('s_feats has %d rows for %d canonical vertices' % (descriptors[0].shape[0], len(V)))
            if live_vertices is not None and descriptors[1].shape[0] != len(live_vertices):
                raise ValueError('l_feats has %d rows for %d live vertices' % (descriptors[1].shape[0], len(live_vertices)))
        if by_descriptor:
            if descriptors is not None and live_vertices is not None:
                lverts, lfaces = np.asarray(live_vertices, dtype=np.float64), None
            else:
                lverts, lfaces = self.marching_cubes(curr_tsdf, step_size=1)[:2]
            if descriptors is not None:
                s_feats, l_feats = descriptors
            else:
                s_feats = self.descriptor_fn(np.asarray(self._vertices), getattr(self, '_faces', None))      # :280
                l_feats = self.descriptor_fn(lverts, lfaces)                                                 # :281
                _solve.check_descriptor_pair(s_feats, l_feats)
                if s_feats.shape[0] != len(V):
                    raise ValueError('s_feats has %d rows for %d canonical vertices' % (s_feats.shape[0], len(V)))
            if l_feats.shape[0] != len(lverts):
                raise ValueError('l_feats has %d rows for %d live vertices' % (l_feats.shape[0], len(lverts)))
            idx = _solve.nearest_descriptors(s_feats, l_feats).to(torch.int64)                               # :282-284
            vp, wn = _solve.warp_points(V, Nn, np.asarray(self._lw, dtype=np.float64), nbr=nbr, node_dq=dq, node_pos=pos, node_w=w)
            found = idx >= 0
            corr = torch.where(found[:, None], _solve._f64(lverts, (3,))[idx.clamp(min=0)], vp)             # :285
            d = vp - corr
            cost = ((wn[:, 0] * d[:, 0] + wn[:, 1] * d[:, 1]) + wn[:, 2] * d[:, 2]).abs()                    # :294
            keep = found & ~(cost > tolerance)                                                              # :295
        elif method == 'sdf':
            # the volume data term (dfh_gn_associate_volume): every warped vertex takes one Newton step along the live volume's
            # trilinear gradient onto its zero level set -- no marching cubes of the live volume, no search; vertices whose cell
            # is not inside the truncation band (or has no usable gradient) get no correspondence and are the ones pruned
            sv = _solve.WarpSolver(knn=nbr.shape[1], distributed=False)
            sv.set_graph(pos, dq, w)
            sv.set_samples(V, Nn, nbr=nbr, sort=False)
            sv.associate_volume(self._live_to_device(curr_tsdf), np.asarray(self._lw, dtype=np.float64), band=self._tdist)
            corr, keep = sv.corr, sv.valid
        else:
            lverts = self.marching_cubes(curr_tsdf, step_size=1)[0] if live_vertices is None else np.asarray(live_vertices)
            if len(lverts) < self._knn:
                raise ValueError('fewer live vertices than knn')
            vp, wn = _solve.warp_points(V, Nn, np.asarray(self._lw, dtype=np.float64), nbr=nbr, node_dq=dq, node_pos=pos, node_w=w)
            corr, cost, keep = _solve.closest_correspondences(vp, wn, np.asarray(lverts, dtype=np.float64), self._knn, tolerance)
        corr = corr.cpu().numpy()
        keep = keep.cpu().numpy().astype(bool)
        self._correspondences = corr
        if prune_result:
            if self._verbose:
                print('ratio of correspondence outlier rejection', float((~keep).sum()) / float(len(V)))
            self._vertices = np.asarray(self._vertices)[keep]
            self._correspondences = corr[keep]
            self._neighbor_look_up = nbr[keep]
            self._normals = np.asarray(self._normals)[keep]
            self._faces = None
            if len(self._vertices) > 0 and getattr(self, '_radius', None) is not None:
                # every node re-anchored on its nearest remaining vertex (dfh_nearest_points)
                npos = np.array([np.asarray(nd[1], dtype=np.float64) for nd in self._nodes])
                vidx = _graph.nearest_points(npos, np.asarray(self._vertices, dtype=np.float64)).cpu().numpy()
                for i in range(len(self._nodes)):
                    nd = self._nodes[i]
                    self._nodes[i] = (int(vidx[i]), nd[1], nd[2], 2 * self._radius)

    def solve(self, correspondences=None, method='cnn', precompute_lw=True, tukey_data_weight=0.2,
              huber_regularization_weight=0.001, regularization_weight=1, iterations=10, pcg_iters=30, huber_delta=1.0):
        """Estimate the warp field {dg_SE3} for the current correspondences; call surface of
        reference core/fusion.py:327-412.  The reference hands `computef` to scipy's trust-region
        solver with finite-difference Jacobians; here the same cost 0.5*|computef|^2 is minimised
        by Levenberg-Marquardt on 6-DoF twists with analytic Jacobians (HIP kernels), under the Huber loss the
        reference passes to scipy (`loss='huber'`, f_scale 1 -> huber_delta = 1, data rows; :389).  Kept from
        the reference: the optional global `_lw` pre-fit on `computef_lw` (:350-364) and the /8
        relaxation of `regularization_weight` while the cost reduction stays in (5 %, 90 %)
        (:405-412), and -- with method='clpts' and no explicit correspondences -- the re-association against
        the stored live volume after the `_lw` pre-fit and before every later round (:364-365, :370-371).  method='sdf': the
        same three-round schedule with setupCorrespondences(method='sdf') as the re-association."""
        if correspondences is not None:
            self._correspondences = correspondences
        reassociate = method in ('clpts', 'sdf') and correspondences is None and self._curr_tsdf is not None
        V, Nn, nbr, C = self._vertex_state()
        pos, dq, w, vidx = self.node_arrays()
        self._itercounter += 1
        if precompute_lw:
            # x' = W(lw, x1): the rigid GN on the pre-warped points is exactly computef_lw's problem
            x1, n1 = self._blend_warp_batch(V, Nn, nbr)
            lw, _ = _solve.solve_rigid_gn(np.asarray(self._lw, dtype=np.float64), x1, n1, C, iters=iterations)
            self._lw = lw
            if reassociate:
                self.setupCorrespondences(self._curr_tsdf, method=method)        # :364-365 (may prune vertices)
        rounds = 3 if method in ('clpts', 'sdf') else 1

        def make_solver():
            V, Nn, nbr, C = self._vertex_state()
            pos, dq, w, vidx = self.node_arrays()
            s_ = _solve.WarpSolver(knn=nbr.shape[1], pcg_iters=pcg_iters)
            s_.set_graph(pos, dq, w, node_nbr=nbr[vidx])
            s_.set_samples(V, Nn, nbr=nbr)
            s_.set_correspondences(C)
            if float(self.landmark_weight) > 0.0:
                # the correspondences as 3-D constraints beside their point-to-plane rows (with method='cnn' and descriptors: the
                # feature matches of setupCorrespondences, which are what stops motion inside the surface)
                s_.landmark_weight = float(self.landmark_weight)
                s_.set_landmarks(V, C, nbr=nbr)
            return s_

        sv = make_solver()
        self.last_costs = []
        for rnd in range(rounds):
            if rnd > 0 and reassociate:
                self._write_back(sv)
                self.setupCorrespondences(self._curr_tsdf, method=method)        # :370-371
                sv = make_solver()
            costs = sv.solve_lm(np.asarray(self._lw, dtype=np.float64), regularization_weight, iters=iterations, lm_abs=1e-3,
                                huber=huber_delta)
            self.last_costs.append(costs)
            cost_before, cost_after = costs[0], costs[-1]
            reduct_rate = (cost_before - cost_after) / cost_before if cost_before > 0 else 0.0
            if reduct_rate > 0.05 and reduct_rate < 0.9:
                regularization_weight /= 8                                      # :407-408
            else:
                break
        self._write_back(sv)

    def _write_back(self, sv):
        new_dq = sv.node_dq.cpu().numpy()
        for idx in range(len(self._nodes)):                                     # :400-403
            nd = self._nodes[idx]
            self._nodes[idx] = (nd[0], nd[1], new_dq[idx], nd[3])

    def _blend_warp_batch(self, V, Nn, nbr):
        """(x1, n1): vertices / normals warped by the blended node DQs only, on the device (dfh_warp_points with an
        identity `_lw`: the identity warp returns its float32-rounded input exactly, and that rounding is the one the
        rigid fit applies to its points anyway, `core/util.py:69`)."""
        pos, dq, w, _ = self.node_arrays()
        ident = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
        return _solve.warp_points(V, Nn, ident, nbr=nbr, node_dq=dq, node_pos=pos, node_w=w)

    # ------------------------------------------------------------------ surface
    def marching_cubes(self, tsdf=None, step_size=0):
        """Reference core/fusion.py:554-568: `measure.marching_cubes_lewiner(volume, step_size=...,
        allow_degenerate=False)` with skimage's default level (min + max) / 2; step_size < 1 means
        `_marching_cubes_step_size`.  GPU mesh extraction of csrc/dfh_mesh.hip (see mesh.py)."""
        return self._marching_cubes(tsdf, step_size)

    def _write_mesh(self, fpath, verts, faces, normals, colors=None, valid=None):
        self._write_mesh_file(fpath, verts, faces, normals, None if colors is None else _mesh.obj_colors(colors, valid, len(verts)))

    @staticmethod
    def _write_mesh_file(fpath, verts, faces, normals, rgb=None):
        """Reference core/fusion.py:577-587: index-space OBJ, `v` / `vn` / `f a b c` (1-based); rgb: vertex-colour columns."""
        with open(fpath, 'w') as f:
            if rgb is None:
                f.write("".join('v %f %f %f\n' % (v[0], v[1], v[2]) for v in verts))
            else:
                f.write("".join('v %f %f %f %f %f %f\n' % (v[0], v[1], v[2], c[0], c[1], c[2]) for v, c in zip(verts, rgb)))
            f.write("".join('vn %f %f %f\n' % (n[0], n[1], n[2]) for n in normals))
            f.write("".join('f %d %d %d\n' % (t[0] + 1, t[1] + 1, t[2] + 1) for t in faces))

    def render_canonical(self, lws, H, W, K=None, scale=1.0, center=np.zeros(3), **kw):
        """The canonical volume ray-cast into the views `lws` (one 3x4 world->camera matrix or a list): a CANONICAL-space view, no
        warp field is applied (the live-frame view of the warped model is render_live_frame).  Voxels are mapped to world by K1's
        rule (scale, center, half = canonical resolution / 2).  K defaults to `_K`.  Returns kernels.raycast's result, with .color
        when there is a colour volume; **kw goes to kernels.raycast."""
        if K is None:
            K = getattr(self, '_K', None)
        if K is None:
            raise ValueError('render_canonical needs the intrinsics: pass K or set _K')
        return self._raycast_canonical(lws, H, W, np.asarray(K, dtype=np.float64), scale, center, **kw)

    def average_edge_dist_in_face(self, f):
        """Reference core/fusion.py:593-597.  (Not shared with FusionDM: this one measures in float64, that one in the vertices'
        own dtype, and the results differ in the last bits.)"""
        v1, v2, v3 = (np.asarray(self._vertices[i], dtype=np.float64) for i in f[:3])
        d = lambda a, b: float(np.sqrt(np.sum((a - b) ** 2)))
        return (d(v1, v2) + d(v1, v3) + d(v2, v3)) / 3

    def fuseDepths(self, dm, lw, tsdf, tsdfw, wmax=100.0, scale=1.0, center=np.zeros(3)):
        """Integrate one depth map into (tsdf, tsdfw).  The reference's Fusion.fuseDepths (core/fusion.py:127-150) does not run
        at HEAD (`current_dm`, a three-argument project_to_pixel, a distance that mixes camera and index coordinates); what it
        sets out to do is what FusionDM.fuseDepths does (core/fusion_dm.py:180-217), so this method IS that sweep (K1,
        dfh_integrate_depth) with the intrinsics given to InitializeCanonicalSpace -- numpy volumes updated in place and
        returned, CUDA tensors updated in place."""
        if getattr(self, '_K', None) is None:
            raise ValueError('fuseDepths needs the intrinsics: call InitializeCanonicalSpace(..., K=K) first')
        lw = np.asarray(lw, dtype=np.float64)
        if lw.shape != (3, 4):
            raise ValueError('lw must be a 3x4 camera extrinsic')
        self._check_volume_pair(tsdf, tsdfw)     # (first: a mismatched pair is refused before the map is looked at)
        dmn = dm if _is_tensor(dm) else np.asarray(dm)
        if dmn.ndim != 2 if not _is_tensor(dm) else dm.dim() != 2:
            raise ValueError('depth map must be 2-D')
        return self._fuse_depth_into(depths_to_device([dmn])[0], lw, tsdf, tsdfw, scale, center, wmax)

    def InitializeCanonicalSpace(self, tsdf=None, depths=None, lws=None, K=None, tsdf_size=256, scale=1.0, center=np.zeros(3),
                                 colors=None, color_band=1.5):
        """The canonical volume from a given TSDF or from depth maps, then the initial mesh and deformation graph: what the
        reference's method of this name sets out to do (core/fusion.py:73-99; at HEAD it reads an undefined `tsdf.shape`, calls a
        free `fuseDepths` and iterates `len(depths)`).  From depth maps: the volume starts at +tdist with weight 0
        (core/fusion.py:80, core/fusion_dm.py:100-101) and the views are fused in order in ONE sweep of the volume
        (dfh_integrate_depth with all the views: the same bits as one fuseDepths call per view, FusionDM.compute_live_tsdf's loop,
        core/fusion_dm.py:166-170).  scale / center: FusionDM.fuseDepths' voxel -> world map (defaults as there).
        colors (with depths): one uint8 image per depth map, averaged into a fresh colour volume `_C` with no warp on the voxels
        within color_band voxels of the surface (kernels.integrate_color)."""
        if colors is not None and (depths is None or len(colors) != len(depths)):
            raise ValueError('colors needs depths, one colour image per depth map')
        if tsdf is not None:
            if not _is_tensor(tsdf) and (type(tsdf) is not np.ndarray or tsdf.ndim != 3):
                raise ValueError('Only 3D numpy array is accepted as tsdf')
            self._T = to_device(tsdf, dtype=self._vol_dtype)
            self._tsdf_host = None
            self._Wt = torch.zeros_like(self._T)                                   # :74
        elif depths is not None and lws is not None and K is not None:
            if len(depths) != len(lws):
                raise ValueError('length of camera matrix array must equal that of depth maps')
            self._K = np.asarray(K, dtype=np.float64)
            self._Kinv = np.linalg.inv(self._K)
            require_gpu()
            R = int(tsdf_size)
            self._T = torch.empty((R, R, R), dtype=self._vol_dtype, device="cuda")
            self._Wt = torch.empty_like(self._T)
            self._tsdf_host = None
            depths, colors, color_depths = self._prepare_depths(depths, colors)
            ds = depths_to_device(depths)        # (one dtype per call: integrate_depth_views wants that)
            kernels.integrate_depth_views(self._T, self._Wt, ds, self._K, self._Kinv, [np.asarray(m, dtype=np.float64) for m in lws],
                                          scale, center, self._tdist, fresh=float(self._tdist))
            self._C = None
            if colors is not None and len(ds) > 0:
                self._C = kernels.color_volume((R, R, R))
                kernels.integrate_color(self._C, self._T, self._Wt, ds if color_depths is None else color_depths, colors, self._K,
                                        self._Kinv, [np.asarray(m, dtype=np.float64) for m in lws], scale, center, self._tdist, color_band)
        else:
            raise ValueError('InitializeCanonicalSpace needs a tsdf, or depths, lws and K')
        if K is not None and getattr(self, '_K', None) is None:
            self._K = np.asarray(K, dtype=np.float64)
            self._Kinv = np.linalg.inv(self._K)
        self._workspace_key = None
        self.initialize_canonical()

    def initialize_canonical(self):
        """What the reference's constructor does after storing the volume (core/fusion.py:86-96): initial
        marching cubes, `_radius` = subsample_rate x mean edge length of the faces, deformation graph.
        Separate from __init__ here so that constructing the object does not need a GPU."""
        self.marching_cubes()
        V = np.asarray(self._vertices)                                           # fp32, as skimage returns them
        F = np.asarray(self._faces)
        if len(F) == 0:
            raise ValueError('marching cubes found no surface in the canonical volume')
        e = (np.linalg.norm(V[F[:, 0]] - V[F[:, 1]], axis=1) + np.linalg.norm(V[F[:, 0]] - V[F[:, 2]], axis=1) +
             np.linalg.norm(V[F[:, 1]] - V[F[:, 2]], axis=1)) / 3                 # average_edge_dist_in_face, :592-596
        self._radius = self._subsample_rate * np.average(e)                      # :92
        self.construct_graph()
