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
import os

import numpy as np
import torch

from . import graph as _graph, io as _io, kernels, mesh as _mesh, solve as _solve
from .device import f32_exact, require_gpu, to_device, torch_dtype


def _is_tensor(a):
    return isinstance(a, torch.Tensor)


class Fusion:
    graph_sampler = "host"       # where construct_graph / update_graph run the radius subsampling (graph.SAMPLERS); set on an instance
    descriptor_fn = None         # a callable (vertices (n,3), faces (m,3) or None) -> (n, D) float32 per-vertex descriptors: stands where
                                 # the reference calls compute_correspondence(self.input, self._feature, self._sess, vertices, faces)
                                 # (core/fusion.py:280-281); with it setupCorrespondences(method='cnn') takes the reference's CNN branch
                                 # (descriptors.PooledDescriptors(feature_fn) is that function around a per-pixel feature network)
    ingest = None                # an ingest.RGBDIngest: the same methods then take the sensor's RAW frames (uint16 depth maps, raw colour
                                 # images) and run them through the stage first, in front of depth_prep; K must equal ingest.K
    depth_prep = None            # a depth_prep.DepthPrep: the methods that sweep a LIST of depth maps (InitializeCanonicalSpace from
                                 # maps, updateTSDF_depths) clean the list with it first; the single-map fuseDepths stays raw

    def __init__(self, tsdf, trunc_distance, subsample_rate=5.0, knn=4, marching_cubes_step_size=3, verbose=False,
                 use_cnn=False, write_warpfield=True, volume_dtype=np.float32):
        if not _is_tensor(tsdf) and (type(tsdf) is not np.ndarray or tsdf.ndim != 3):
            raise ValueError('Only 3D numpy array is accepted as tsdf')          # core/fusion.py:51-52
        if _is_tensor(tsdf) and tsdf.dim() != 3:
            raise ValueError('Only 3D numpy array is accepted as tsdf')
        if use_cnn:
            raise NotImplementedError('the CNN correspondence branch (core/sdf.py:75-150) is outside this hot path')
        self._itercounter = 0
        self._curr_tsdf = None
        self._tdist = abs(trunc_distance)
        self._lw = np.array([1, 0, 0, 0, 0, 0.1, 0, 0], dtype=np.float32)        # :57
        self._knn = knn
        self._marching_cubes_step_size = marching_cubes_step_size
        self._subsample_rate = subsample_rate
        self._nodes = []
        self._neighbor_look_up = []
        self._correspondences = []
        self.landmark_weight = 0.0               # > 0: solve() also uses the correspondences as POINTS (WarpSolver.set_landmarks)
        self.min_component_faces = None          # a number: marching_cubes() drops the components with fewer faces from the stored mesh
        self.simplify_cell = None                # a number: write_canonical_mesh() writes the mesh clustered at that cell size (voxels)
        self._vertices = None
        self._normals = None
        self._kdtree = None
        self._verbose = verbose
        self._write_warpfield = write_warpfield
        self._sess = None
        self._vol_dtype = torch_dtype(volume_dtype)
        self._T = None
        self._Wt = None
        self._tsdf_host = tsdf                   # uploaded on first use (ctor works without a GPU)
        self._workspace = None
        self._workspace_key = None
        self._C = None                           # the colour volume (kernels.color_volume): set by the calls given colour images

    # ------------------------------------------------------------------ volumes
    def _ensure_volumes(self):
        if self._T is None:
            require_gpu()
            self._T = to_device(self._tsdf_host, dtype=self._vol_dtype)
            self._tsdf_host = None
        if self._Wt is None:
            self._Wt = torch.zeros_like(self._T)                                 # InitializeCanonicalSpace, :74

    @property
    def _tsdf(self):
        self._ensure_volumes()
        return self._T.cpu().numpy().astype(np.float64)

    @_tsdf.setter
    def _tsdf(self, value):
        self._T = to_device(value, dtype=self._vol_dtype)
        self._tsdf_host = None

    @property
    def _tsdfw(self):
        self._ensure_volumes()
        return self._Wt.cpu().numpy().astype(np.float64)

    @_tsdfw.setter
    def _tsdfw(self, value):
        self._Wt = to_device(value, dtype=self._vol_dtype)

    @property
    def tsdf_device(self):
        self._ensure_volumes()
        return self._T, self._Wt

    # ------------------------------------------------------------------ graph
    def node_arrays(self):
        """(pos (N,3), dq (N,8), w (N,), vertex index (N,)) from the `_nodes` 4-tuples."""
        if len(self._nodes) == 0:
            raise ValueError('the deformation graph is empty: fill _nodes first')
        vidx = np.array([int(n[0]) for n in self._nodes], dtype=np.int64)
        pos = np.array([np.asarray(n[1], dtype=np.float64) for n in self._nodes])
        dq = np.array([np.asarray(n[2], dtype=np.float64) for n in self._nodes])
        w = np.array([float(n[3]) for n in self._nodes], dtype=np.float64)
        return pos, dq, w, vidx

    def _live_to_device(self, curr_tsdf):
        if _is_tensor(curr_tsdf):
            if curr_tsdf.dim() != 3:
                raise ValueError('Only accept 3D np array as tsdf')
            t = curr_tsdf if curr_tsdf.dtype in (torch.float32, torch.float64) else curr_tsdf.to(torch.float32)
            return to_device(t)
        if type(curr_tsdf) is not np.ndarray:
            raise ValueError('Only accept 3D np array as tsdf')                  # :160-161
        if curr_tsdf.ndim != 3:
            raise ValueError('Only accept 3D np array as tsdf')                  # :162-163
        return to_device(curr_tsdf, dtype=torch.float32 if f32_exact(curr_tsdf) else torch.float64)

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
        res = tuple(self._T.shape)
        key = (res, pos.tobytes(), w.tobytes(), self._knn)          # what the workspace's stored indices / weights depend on
        rebuild = key != self._workspace_key
        if rebuild:
            self._workspace = kernels.dqb_workspace(res, knn=self._knn, n_nodes=len(pos))
            self._workspace_key = key
        kernels.fuse_volume_dqb(self._T, self._Wt, live, pos, dq, w, self._knn,
                                np.asarray(self._lw, dtype=np.float64), self._tdist, wmax,
                                workspace=self._workspace, rebuild_candidates=rebuild)

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
        color_depths = None
        if self.ingest is not None and depths:                       # raw frames in; the colour fusion reads the colour-only maps
            depths, colors, color_depths = self.ingest.frame(depths, colors, K=self._K)
        if self.depth_prep is not None and depths:
            depths = self.depth_prep(depths, self._Kinv, want_normals=False)[0]

        def exact32(d):
            return (d.dtype == torch.float32) if _is_tensor(d) else f32_exact(np.asarray(d))
        ddt = torch.float32 if all(exact32(d) for d in depths) else torch.float64
        ds = [to_device(d if _is_tensor(d) else np.asarray(d), dtype=ddt) for d in depths]
        self._ensure_volumes()
        pos, dq, w, _ = self.node_arrays()
        res = tuple(self._T.shape)
        key = (res, pos.tobytes(), w.tobytes(), self._knn)          # shared with updateTSDF: one workspace serves both
        rebuild = key != self._workspace_key
        if rebuild:
            self._workspace = kernels.dqb_workspace(res, knn=self._knn, n_nodes=len(pos))
            self._workspace_key = key
        kernels.integrate_depth_dqb(self._T, self._Wt, ds, self._K, self._Kinv, lws, scale, center, self._tdist, pos, dq, w,
                                    self._knn, np.asarray(self._lw, dtype=np.float64), wmax=wmax, weight=weight,
                                    tsdf_res=res[0], workspace=self._workspace, rebuild_candidates=rebuild)
        if colors is not None:
            if self._C is None:
                self._C = kernels.color_volume(res)
            kernels.integrate_color(self._C, self._T, self._Wt, ds if color_depths is None else color_depths, colors, self._K,
                                    self._Kinv, lws, scale, center, self._tdist, color_band, pos, dq, w, self._knn, np.asarray(self._lw, dtype=np.float64), tsdf_res=res[0],
                                    workspace=self._workspace,
                                    stored_indices=kernels.dqb_has_indices(self._workspace, res, self._knn, len(pos)))

    # ------------------------------------------------------------------ A5 (single-point helpers)
    def _gather_nodes(self, locations, dqs):
        pos, dq, w, _ = self.node_arrays()
        loc = np.asarray(locations, dtype=np.int64)
        dq_k = dq[loc] if dqs is None else np.asarray([np.asarray(d, dtype=np.float64) for d in dqs])
        return loc, pos[loc], dq_k, w[loc]

    def _locations(self, pos, k):
        node_pos = self.node_arrays()[0]
        nbr, _ = _solve.sample_knn(np.asarray(pos, dtype=np.float64)[None, :], node_pos, np.ones(len(node_pos)), k)
        return nbr[0].cpu().numpy()

    def dq_blend(self, pos, dqs=None, locations=None, dmax=None):
        """Blend the DQs of the given (or the knn nearest) nodes at `pos`; reference
        core/fusion.py:527-551.  Single points are host arithmetic; volumes and vertex sets go
        through updateTSDF / computef."""
        if dqs is None or locations is None:
            locations = self._locations(pos, self._knn)                          # :529
            dqs = None
        loc, npos, dq_k, w_k = self._gather_nodes(locations, dqs)
        pos = np.asarray(pos)
        dqb = np.zeros(8)
        for j in range(len(loc)):
            dist = np.sqrt(np.sum((pos.astype(np.float64) - npos[j]) ** 2))
            sig = 2 * w_k[j] if dmax is None else dmax
            dqb = dqb + np.exp(-1.0 * (dist / sig) ** 2) * dq_k[j]              # :537-541
        n = np.sqrt(np.sum(dqb * dqb))
        if n == 0:
            return np.array([1, 0, 0, 0, 0, 0, 0, 0], dtype=np.float32)          # :544-549
        return dqb / n

    @staticmethod
    def _dqb_warp(dq, p):
        from .dq import qmul
        dq = np.asarray(dq, dtype=np.float64)
        p = np.asarray(p).astype(np.float32).astype(np.float64)                  # util.py:69
        r, d = dq[:4], dq[4:]
        rc = r * np.array([1.0, -1.0, -1.0, -1.0])
        return (qmul(qmul(r, np.append(0.0, p)), rc) + 2.0 * qmul(d, rc))[1:]

    def warp(self, pos, dqs=None, locations=None, normal=None, dmax=None, m_lw=None):
        """Warp one point (and normal) from canonical space to the live frame; reference
        core/fusion.py:502-520."""
        if dqs is None or locations is None:
            locations = self._locations(pos, self._knn + 1)[:-1]                 # :504-505
            dqs = None
        se3 = self.dq_blend(pos, dqs if dqs is not None else [self._nodes[i][2] for i in locations], locations, dmax)
        pos_warped = self._dqb_warp(se3, pos)
        if m_lw is not None:
            pos_warped = self._dqb_warp(m_lw, pos_warped)
        if normal is None:
            return pos_warped
        rq = np.append(np.asarray(se3, dtype=np.float64)[:4], [0, 0, 0, 0])
        normal_warped = self._dqb_warp(rq, normal)
        if m_lw is not None:
            normal_warped = self._dqb_warp(np.append(np.asarray(m_lw, dtype=np.float64)[:4], [0, 0, 0, 0]), normal_warped)
        return (pos_warped, normal_warped)

    # ------------------------------------------------------------------ A10
    def _vertex_state(self):
        if self._vertices is None or self._normals is None or len(self._neighbor_look_up) == 0:
            raise ValueError('canonical vertices / normals / _neighbor_look_up have not been set')
        V = np.asarray(self._vertices, dtype=np.float64)
        Nn = np.asarray(self._normals, dtype=np.float64)
        nbr = np.asarray(self._neighbor_look_up, dtype=np.int64)
        C = np.asarray(self._correspondences, dtype=np.float64)
        if len(C) != len(V):
            raise ValueError("Please first call setupCorrespondences to compute point to point correspondences "
                             "between canonical and live frame vertices!")      # :337-338
        return V, Nn, nbr, C

    def computef_lw(self, x, tdw, trw):
        """Data rows with the global transform `x` in place of `_lw`; reference core/fusion.py:444-456."""
        V, Nn, nbr, C = self._vertex_state()
        pos, dq, w, _ = self.node_arrays()
        return _solve.residual_data(dq, V, Nn, C, nbr, pos, w, x).cpu().numpy()

    def computef(self, x, tdw, trw, rw):
        """Residual vector [data rows | regularisation rows] for the flattened node DQs `x`;
        reference core/fusion.py:459-491 (tdw / trw are unused there too)."""
        V, Nn, nbr, C = self._vertex_state()
        pos, _, w, vidx = self.node_arrays()
        dqs = np.asarray(x, dtype=np.float64).reshape(-1, 8)
        if len(dqs) != len(pos):
            raise ValueError('x must hold 8 values per deformation node')
        fd = _solve.residual_data(dqs, V, Nn, C, nbr, pos, w, self._lw)
        fr = _solve.residual_reg(dqs, nbr[vidx], pos, w, rw)
        return torch.cat([fd, fr]).cpu().numpy()

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

    def computeSparsity(self, n, m):
        """Jacobian sparsity of `computef` for a solver that wants it (reference core/fusion.py:416-442): data row
        idx touches the 8 DQ entries of each of its k nodes; the three regularisation rows of node idx touch node
        idx and the nodes in the look-up row of its anchor vertex.  (Only the first of the node's k regulariser
        triples is marked there -- reproduced; this build's own solver does not use it.)"""
        from scipy.sparse import coo_matrix
        nbr = np.asarray(self._neighbor_look_up, dtype=np.int64)
        V = len(self._vertices)
        N = len(self._nodes)
        e8 = np.arange(8)
        rows = [np.repeat(np.arange(V), nbr.shape[1] * 8)]
        cols = [(8 * nbr[:, :, None] + e8).reshape(-1)]
        vidx = np.array([int(nd[0]) for nd in self._nodes], dtype=np.int64)
        node_cols = np.concatenate([np.arange(N)[:, None], nbr[vidx]], axis=1)            # (N, 1+k)
        r3 = V + 3 * np.arange(N)[:, None] + np.arange(3)                                 # (N, 3)
        rows.append(np.repeat(r3.reshape(-1), node_cols.shape[1] * 8))
        cols.append(np.tile((8 * node_cols[:, :, None] + e8).reshape(N, 1, -1), (1, 3, 1)).reshape(-1))
        r, c = np.concatenate(rows), np.concatenate(cols)
        mat = coo_matrix((np.ones(len(r), dtype=np.float32), (r, c)), shape=(n, m)).tocsr()       # duplicates add up:
        mat.data[:] = 1.0                                                                          # entries are flags
        return mat.tolil()

    def write_live_frame_mesh(self, path, filename, warpfield_path):
        """Reference core/fusion.py:588-590 ("Process a warp field file and write the live frame mesh"; an empty stub there): the
        canonical mesh warped into the live frame (live_frame_mesh) with the nodes of `warpfield_path` (a file of
        write_warp_field; None / "" = the current `_nodes`), written in write_canonical_mesh's layout.  Returns the file path."""
        nodes = _io.read_warp_field(warpfield_path) if warpfield_path else None
        verts, faces, normals = self.live_frame_mesh(nodes)
        fpath = os.path.join(path, filename)
        self._write_mesh_file(fpath, verts.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy())
        return fpath

    def live_frame_mesh(self, nodes=None):
        """The canonical surface in the live frame, on the device: (verts (V,3) fp64, faces (F,3) int32, normals (V,3) fp64) CUDA
        tensors.  Marching cubes of the canonical volume as write_canonical_mesh extracts it, each vertex's `_knn` nearest nodes
        (solve.sample_knn), then the warp of solve()'s data term -- reference `warp(v, normal=n, m_lw=_lw)` per vertex
        (solve.warp_points).  nodes: reference-shaped 4-tuples (vertex index, position, DQ, weight) as io.read_warp_field returns
        them; None = `_nodes`.  With no nodes only `_lw` is applied."""
        self._ensure_volumes()
        verts, faces, normals = self._canonical_mesh_device()
        nodes = self._nodes if nodes is None else nodes
        lw = np.asarray(self._lw, dtype=np.float64)
        if len(nodes) == 0:
            vp, vn = _solve.warp_points(verts, normals, lw)
            return vp, faces, vn
        pos = np.array([np.asarray(n[1], dtype=np.float64) for n in nodes]).reshape(-1, 3)
        dq = np.array([np.asarray(n[2], dtype=np.float64) for n in nodes]).reshape(-1, 8)
        w = np.array([float(n[3]) for n in nodes], dtype=np.float64)
        if len(pos) < self._knn:
            raise ValueError('the warp field has %d nodes, fewer than knn = %d' % (len(pos), self._knn))
        if verts.shape[0] == 0:
            return verts.to(torch.float64), faces, normals.to(torch.float64)
        nbr, _ = _solve.sample_knn(verts, pos, w, self._knn)
        vp, vn = _solve.warp_points(verts, normals, lw, nbr=nbr, node_dq=dq, node_pos=pos, node_w=w)
        return vp, faces, vn

    def render_live_frame(self, lws, H, W, K=None, scale=1.0, center=np.zeros(3), nodes=None):
        """Depth / normal / face-id maps of live_frame_mesh(nodes) in the views `lws` (one 3x4 world->camera matrix or a list; one
        launch), voxels mapped to world by K1's rule (scale, center, half = canonical resolution / 2).  K defaults to `_K`.
        Returns mesh.render's (depth, normal, face)."""
        if K is None:
            K = getattr(self, '_K', None)
        if K is None:
            raise ValueError('render_live_frame needs the intrinsics: pass K or set _K')
        verts, faces, normals = self.live_frame_mesh(nodes)
        half = self._T.shape[0] / 2.0
        return _mesh.render(verts, faces, normals, K, lws, H, W, scale=scale, center=center, half=half)

    def render_canonical(self, lws, H, W, K=None, scale=1.0, center=np.zeros(3), **kw):
        """The canonical volume ray-cast into the views `lws` (one 3x4 world->camera matrix or a list): a CANONICAL-space view, no
        warp field is applied (the live-frame view of the warped model is render_live_frame).  Voxels are mapped to world by K1's
        rule (scale, center, half = canonical resolution / 2).  K defaults to `_K`.  Returns kernels.raycast's result, with .color
        when there is a colour volume; **kw goes to kernels.raycast."""
        if K is None:
            K = getattr(self, '_K', None)
        if K is None:
            raise ValueError('render_canonical needs the intrinsics: pass K or set _K')
        K = np.asarray(K, dtype=np.float64)
        self._ensure_volumes()
        lws = [lws] if np.asarray(lws[0]).ndim == 1 else list(lws)
        if self._C is not None:
            kw.setdefault("colors", self._C)
            kw.setdefault("want", ("depth", "normals", "color"))
        return kernels.raycast(self._T, self._Wt, K, np.linalg.inv(K), lws, H, W, scale, center, tsdf_res=self._T.shape[0], **kw)

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

    # ------------------------------------------------------------------ graph maintenance (§8(f) rank 3)
    def marching_cubes(self, tsdf=None, step_size=0):
        """Reference core/fusion.py:554-568: `measure.marching_cubes_lewiner(volume, step_size=...,
        allow_degenerate=False)` with skimage's default level (min + max) / 2; step_size < 1 means
        `_marching_cubes_step_size`.  GPU mesh extraction of csrc/dfh_mesh.hip (see mesh.py)."""
        if step_size < 1:
            step_size = self._marching_cubes_step_size
        if tsdf is not None:
            return _mesh.marching_cubes(self._live_to_device(tsdf), None, step_size, as_numpy=True)
        self._ensure_volumes()
        if self.min_component_faces is None:
            self._vertices, self._faces, self._normals, values = _mesh.marching_cubes(self._T, None, step_size, as_numpy=True)
        else:                                    # the mesh without its fragments (mesh.filter_components), cleaned on the device
            v, f, n, _ = _mesh.marching_cubes(self._T, None, step_size)
            v, f, n, _ = _mesh.filter_components(v, f, n, min_faces=self.min_component_faces)
            self._vertices, self._faces, self._normals = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()
        if self._verbose:
            print("Marching Cubes result: number of extracted vertices is %d" % (len(self._vertices)))

    def surface_samples(self, tsdf=None, band=1.0):
        """Dense band-voxel samples (csrc/dfh_extract.hip) in place of mesh vertices; not in the reference."""
        from .pipeline import extract_surface_samples
        if tsdf is not None:
            live = self._live_to_device(tsdf)
            pos, nrm = extract_surface_samples(live, torch.ones_like(live), band)
            return pos.cpu().numpy(), None, nrm.cpu().numpy(), None
        self._ensure_volumes()
        w = self._Wt if float(self._Wt.max()) > 0 else torch.ones_like(self._T)
        pos, nrm = extract_surface_samples(self._T, w, band)
        self._vertices, self._faces, self._normals = pos.cpu().numpy(), None, nrm.cpu().numpy()

    def write_canonical_mesh(self, path, filename):
        """Reference core/fusion.py:577-587: index-space OBJ, `v` / `vn` / `f a b c` (1-based)."""
        self._ensure_volumes()
        if self.simplify_cell is not None:   # a coarser file (mesh.simplify); the stored mesh and the graph are not touched
            verts, faces, normals, _ = _mesh.marching_cubes(self._T, None, 1)
            verts, faces, normals, _ = _mesh.simplify_with_normals(verts, faces, normals, self.simplify_cell)
            colors = None
            if self._C is not None:      # the colour volume sampled at the new vertices, not an average of the old colours
                rgb, valid = kernels.sample_colors(self._C, verts.double())
                colors = _mesh.obj_colors(rgb.cpu().numpy(), valid.cpu().numpy(), len(verts))
            self._write_mesh_file(os.path.join(path, filename), verts.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy(), colors)
            return
        if self._C is not None:          # vertex colours (not in the reference): the colour volume sampled at the vertices
            verts, faces, normals, values = _mesh.marching_cubes(self._T, None, 1)
            rgb, valid = kernels.sample_colors(self._C, verts.double())
            self._write_mesh_file(os.path.join(path, filename), verts.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy(),
                                  _mesh.obj_colors(rgb.cpu().numpy(), valid.cpu().numpy(), len(verts)))
            return
        verts, faces, normals, values = _mesh.marching_cubes(self._T, None, 1, as_numpy=True)
        self._write_mesh_file(os.path.join(path, filename), verts, faces, normals)

    def _canonical_mesh_device(self):
        """The extraction of write_canonical_mesh, left on the device: (verts, faces, normals)."""
        verts, faces, normals, _ = _mesh.marching_cubes(self._T, None, 1)
        return verts, faces, normals

    @staticmethod
    def _write_mesh_file(fpath, verts, faces, normals, rgb=None):
        with open(fpath, 'w') as f:
            if rgb is None:
                f.write("".join('v %f %f %f\n' % (v[0], v[1], v[2]) for v in verts))
            else:
                f.write("".join('v %f %f %f %f %f %f\n' % (v[0], v[1], v[2], c[0], c[1], c[2]) for v, c in zip(verts, rgb)))
            f.write("".join('vn %f %f %f\n' % (n[0], n[1], n[2]) for n in normals))
            f.write("".join('f %d %d %d\n' % (t[0] + 1, t[1] + 1, t[2] + 1) for t in faces))

    def average_edge_dist_in_face(self, f):
        """Reference core/fusion.py:593-597."""
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
        if _is_tensor(tsdf) != _is_tensor(tsdfw):
            raise ValueError('tsdf and tsdfw must both be numpy arrays or both CUDA tensors')
        dmn = dm if _is_tensor(dm) else np.asarray(dm)
        if dmn.ndim != 2 if not _is_tensor(dm) else dm.dim() != 2:
            raise ValueError('depth map must be 2-D')
        depth = to_device(dmn, dtype=torch.float32 if (_is_tensor(dm) and dm.dtype == torch.float32) or (not _is_tensor(dm) and f32_exact(dmn))
                          else torch.float64)
        if _is_tensor(tsdf):
            kernels.integrate_depth(tsdf, tsdfw, depth, self._K, self._Kinv, lw, scale, center, self._tdist, wmax, tsdf_res=tsdf.shape[0])
            return (tsdf, tsdfw)
        if tsdf.ndim != 3 or tsdf.shape != tsdfw.shape:
            raise ValueError('tsdf and tsdfw must be 3-D arrays of the same shape')
        T, Wt = to_device(tsdf, dtype=self._vol_dtype), to_device(tsdfw, dtype=self._vol_dtype)
        kernels.integrate_depth(T, Wt, depth, self._K, self._Kinv, lw, scale, center, self._tdist, wmax, tsdf_res=tsdf.shape[0])
        tsdf[...] = T.cpu().numpy()
        tsdfw[...] = Wt.cpu().numpy()
        return (tsdf, tsdfw)

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
            color_depths = None
            if self.ingest is not None and len(depths) > 0:
                depths, colors, color_depths = self.ingest.frame(depths, colors, K=self._K)
            if self.depth_prep is not None and len(depths) > 0:
                depths = self.depth_prep(depths, self._Kinv, want_normals=False)[0]
            # (the dtype rule of fuseDepths: float32 on the device unless a float64 map is not float32-exact -- then every map
            # travels as float64, so that no visibility mask can flip; integrate_depth_views wants one dtype per call)
            def exact32(d):
                return (d.dtype == torch.float32) if _is_tensor(d) else f32_exact(np.asarray(d))
            ddt = torch.float32 if all(exact32(d) for d in depths) else torch.float64
            ds = [to_device(d if _is_tensor(d) else np.asarray(d), dtype=ddt) for d in depths]
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

    def construct_graph(self):
        """Reference core/fusion.py:101-123 (needs `_vertices` and `_radius`).  The vertex -> node table is computed on the
        device (dfh_sample_knn); `_kdtree` is a graph.NodeIndex (device look-ups) in place of the reference's KD-tree.
        `graph_sampler` = "device": the radius subsampling runs on the device as well (same nodes)."""
        _graph._check_sampler(self.graph_sampler)
        if self._vertices is None or getattr(self, '_radius', None) is None:
            raise ValueError('construct_graph needs _vertices and _radius')
        vidx, pos, dq, w, lookup = _graph.construct_graph_device(self._vertices, self._radius, self._knn, sampler=self.graph_sampler)
        self._nodes = [(vidx[i], pos[i], dq[i].copy(), w[i]) for i in range(len(pos))]
        self._kdtree = _graph.NodeIndex(pos)
        self._neighbor_look_up = lookup.cpu().numpy().astype(np.int64)

    def _dq_blend_kdtree(self, pos):
        d, loc = self._kdtree.query(pos, k=self._knn)                       # core/fusion.py:529
        return self.dq_blend(pos, [self._nodes[i][2] for i in np.atleast_1d(loc)], np.atleast_1d(loc))

    def update_graph(self, refresh_surface=True):
        """Reference core/fusion.py:201-239: refresh the surface, re-anchor the nodes, insert nodes
        for unsupported vertices, rebuild the lookup, drop the live-frame data, write the warp field.
        The O(vertices x nodes) steps run on the device (graph.update_graph_device), the subsampling where `graph_sampler` says."""
        _graph._check_sampler(self.graph_sampler)
        if refresh_surface:
            self.marching_cubes()
        pos, dq, w, _ = self.node_arrays()
        vidx, P2, Q2, W2, lookup, n_new = _graph.update_graph_device(pos, dq, w, np.asarray(self._vertices, dtype=np.float64),
                                                                    self._radius, self._knn, sampler=self.graph_sampler)
        vidx, P2, Q2 = vidx.cpu().numpy(), P2.cpu().numpy(), Q2.cpu().numpy()
        old = self._nodes
        N = len(old)
        # old nodes keep their position / DQ objects (:208-212); new ones carry the blend (:222)
        self._nodes = [(vidx[i], old[i][1], old[i][2], 2 * self._radius) for i in range(N)] + \
                      [(vidx[i], P2[i], Q2[i], 2 * self._radius) for i in range(N, len(P2))]
        self._kdtree = _graph.NodeIndex(P2)
        self._neighbor_look_up = lookup.cpu().numpy().astype(np.int64)
        self._curr_tsdf = None
        self._correspondences = []
        self._workspace_key = None
        if self._write_warpfield:
            self.write_warp_field(getattr(self, 'DATA_PATH', '.'), 'test')
        return n_new

    def write_warp_field(self, path, filename):
        """Reference core/fusion.py:571-573."""
        return _io.write_warp_field(self._nodes, path, filename, self._itercounter)


# The reference's FusionDM carries a second copy of the non-rigid methods ("functions below not useful for now",
# core/fusion_dm.py:366-560): computeSparsity, computef, warp, dq_blend, construct_graph, update_graph -- the same statements as
# Fusion's up to white space.  FusionDM here gets the same methods (and the helpers they call) from Fusion, so the call surface
# is complete; like in the reference they need `_nodes`, `_vertices`, `_normals`, `_neighbor_look_up`, `_radius` and one
# correspondence per vertex to be set by the caller.
def _lend_nonrigid_methods():
    from .fusion_dm import FusionDM
    for name in ("node_arrays", "_gather_nodes", "_locations", "dq_blend", "_dqb_warp", "warp", "_vertex_state", "computef",
                 "computeSparsity", "construct_graph", "_dq_blend_kdtree", "update_graph", "live_frame_mesh", "render_live_frame"):
        if name not in FusionDM.__dict__:
            setattr(FusionDM, name, Fusion.__dict__[name])
    if "graph_sampler" not in FusionDM.__dict__:
        FusionDM.graph_sampler = Fusion.graph_sampler


_lend_nonrigid_methods()
