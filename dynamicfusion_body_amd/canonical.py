"""`CanonicalModel`: what `Fusion` (fusion.py) and `FusionDM` (fusion_dm.py) both are -- a canonical TSDF / weight / colour
volume on the device, the mesh taken from it, and a deformation graph over that mesh.  The reference states all of this twice
(core/fusion.py and core/fusion_dm.py); here it is stated once and the two classes derive from it.

One class, not two: the non-rigid methods the reference's FusionDM repeats (see "deformation graph" below) live in the same
base as the volume and mesh code, because they call it (live_frame_mesh -> _canonical_mesh_device, update_graph ->
marching_cubes / write_warp_field) and a second class would only add a line of bases to each subclass.

Where the two classes deliberately differ, the difference is a class attribute or a small method of the subclass:
  `_mc_level`              the level write_canonical_mesh / live_frame_mesh extract at (None: skimage's (min + max) / 2; 0.0)
  `_write_mesh`            the OBJ layout (`f a b c` in index space; `f a//a b//b c//c` in world space through `_IND`)
  `_unit_weight_samples`   whether surface_samples reads a never-fused volume with unit weights
  `_live_tensor_error`, `_weight_arg`   the wording of two ValueErrors (tests match on the texts)
  `_ensure_volumes`        where the volumes come from on first use (the constructor's host array; +tdist / 0)
  marching_cubes' default step, fuseDepths' signature, render_canonical / render_model: thin public methods of each class.
"""
import os

import numpy as np
import torch

from . import graph as _graph, io as _io, kernels, mesh as _mesh, solve as _solve
from .device import f32_exact, to_device, torch_dtype


def _is_tensor(a):
    return isinstance(a, torch.Tensor)


class CanonicalModel:
    graph_sampler = "host"       # where construct_graph / update_graph run the radius subsampling (graph.SAMPLERS); set on an instance
    ingest = None                # an ingest.RGBDIngest: the methods that take a LIST of depth maps then take the sensor's RAW frames
                                 # (uint16 depth maps, raw colour images) and run them through the stage first, in front of
                                 # depth_prep; K must equal ingest.K; set on an instance
    depth_prep = None            # a depth_prep.DepthPrep: the same methods (FusionDM.compute_live_tsdf, Fusion.InitializeCanonicalSpace
                                 # from maps, Fusion.updateTSDF_depths) clean the list with it first; the single-map fuseDepths stays raw

    def _init_model(self, trunc_distance, subsample_rate, knn, marching_cubes_step_size, verbose, write_warpfield, volume_dtype):
        """The attributes both constructors assign (reference core/fusion.py:53-72, core/fusion_dm.py:57-81).  No GPU is touched:
        the volumes are made on first use (_ensure_volumes)."""
        self._itercounter = 0
        self._curr_tsdf = None
        self._tdist = abs(trunc_distance)
        self._knn = knn
        self._marching_cubes_step_size = marching_cubes_step_size
        self._subsample_rate = subsample_rate
        self._nodes = []
        self._neighbor_look_up = []
        self._correspondences = []
        self.min_component_faces = None          # a number: marching_cubes() drops the components with fewer faces from the stored mesh
        self.simplify_cell = None                # a number: write_canonical_mesh() writes the mesh clustered at that cell size (voxels)
        self.smooth_iters = None                 # a number: write_canonical_mesh() writes the mesh after that many Taubin iterations
        self._vertices = None
        self._normals = None
        self._kdtree = None
        self._verbose = verbose
        self._write_warpfield = write_warpfield
        self._vol_dtype = torch_dtype(volume_dtype)
        self._T = None                           # device volumes, made on first use
        self._Wt = None
        self._C = None                           # the colour volume (kernels.color_volume): set by the calls given colour images

    # ------------------------------------------------------------------ volumes
    @property
    def _tsdf(self):
        self._ensure_volumes()
        return self._T.cpu().numpy().astype(np.float64)

    @_tsdf.setter
    def _tsdf(self, value):
        self._T = to_device(value, dtype=self._vol_dtype)

    @property
    def _tsdfw(self):
        self._ensure_volumes()
        return self._Wt.cpu().numpy().astype(np.float64)

    @_tsdfw.setter
    def _tsdfw(self, value):
        self._Wt = to_device(value, dtype=self._vol_dtype)

    @property
    def tsdf_device(self):
        """The resident TSDF / weight tensors (no copy)."""
        self._ensure_volumes()
        return self._T, self._Wt

    def _live_to_device(self, curr_tsdf):
        if _is_tensor(curr_tsdf):
            if curr_tsdf.dim() != 3:
                raise ValueError(self._live_tensor_error)
            t = curr_tsdf if curr_tsdf.dtype in (torch.float32, torch.float64) else curr_tsdf.to(torch.float32)
            return to_device(t)
        if type(curr_tsdf) is not np.ndarray or curr_tsdf.ndim != 3:
            raise ValueError('Only accept 3D np array as tsdf')                  # core/fusion.py:160-163
        return to_device(curr_tsdf, dtype=torch.float32 if f32_exact(curr_tsdf) else torch.float64)

    def _prepare_depths(self, depths, colors):
        """Raw frames -> `ingest` -> `depth_prep`, where set: (depths, colors, color_depths).  color_depths: the colour-only maps
        the colour fusion reads in place of the depth maps (None without an ingest stage)."""
        color_depths = None
        if self.ingest is not None and len(depths) > 0:
            depths, colors, color_depths = self.ingest.frame(depths, colors, K=self._K)
        if self.depth_prep is not None and len(depths) > 0:
            depths = self.depth_prep(depths, self._Kinv, want_normals=False)[0]
        return depths, colors, color_depths

    def _check_volume_pair(self, tsdf, tsdf_w):
        if _is_tensor(tsdf) != _is_tensor(tsdf_w):
            raise ValueError('tsdf and %s must both be numpy arrays or both CUDA tensors' % self._weight_arg)

    def _fuse_depth_into(self, depth, lw, tsdf, tsdf_w, scale, center, wmax, tsdf_res=None):
        """The sweep of fuseDepths (K1, reference core/fusion_dm.py:180-217) once the map is on the device: CUDA volumes are
        updated in place; numpy volumes are uploaded, swept, written back in place AND returned (the reference mutates through
        np.nditer and returns the same arrays, :186,:217).  tsdf_res=None: the volume's own first extent."""
        self._check_volume_pair(tsdf, tsdf_w)
        if _is_tensor(tsdf):
            kernels.integrate_depth(tsdf, tsdf_w, depth, self._K, self._Kinv, lw, scale, center, self._tdist, wmax,
                                    tsdf_res=tsdf.shape[0] if tsdf_res is None else tsdf_res)
            return (tsdf, tsdf_w)
        if tsdf.ndim != 3 or tsdf.shape != tsdf_w.shape:
            raise ValueError('tsdf and %s must be 3-D arrays of the same shape' % self._weight_arg)
        T, Wt = to_device(tsdf, dtype=self._vol_dtype), to_device(tsdf_w, dtype=self._vol_dtype)
        kernels.integrate_depth(T, Wt, depth, self._K, self._Kinv, lw, scale, center, self._tdist, wmax,
                                tsdf_res=tsdf.shape[0] if tsdf_res is None else tsdf_res)
        tsdf[...] = T.cpu().numpy()
        tsdf_w[...] = Wt.cpu().numpy()
        return (tsdf, tsdf_w)

    def _raycast_canonical(self, lws, H, W, K, scale, center, tsdf_res=None, **kw):
        """The body of Fusion.render_canonical / FusionDM.render_model.  tsdf_res=None: the volume's own first extent."""
        self._ensure_volumes()
        lws = [lws] if np.asarray(lws[0]).ndim == 1 else list(lws)
        if self._C is not None:
            kw.setdefault("colors", self._C)
            kw.setdefault("want", ("depth", "normals", "color"))
        return kernels.raycast(self._T, self._Wt, K, np.linalg.inv(K), lws, H, W, scale, center,
                               tsdf_res=self._T.shape[0] if tsdf_res is None else tsdf_res, **kw)

    # ------------------------------------------------------------------ surface
    def _marching_cubes(self, tsdf, step_size):
        """The body of both marching_cubes methods (their defaults for step_size differ)."""
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
        """Dense alternative to the mesh vertices for the solve (not in the reference): every band
        voxel moved onto the zero level set along the TSDF gradient (csrc/dfh_extract.hip), with the
        normalised gradient as normal.  Same shapes as marching_cubes, faces / values = None."""
        from .pipeline import extract_surface_samples
        if tsdf is not None:
            live = self._live_to_device(tsdf)
            pos, nrm = extract_surface_samples(live, torch.ones_like(live), band)
            return pos.cpu().numpy(), None, nrm.cpu().numpy(), None
        self._ensure_volumes()
        w = self._Wt
        if self._unit_weight_samples and not float(w.max()) > 0:
            w = torch.ones_like(self._T)
        pos, nrm = extract_surface_samples(self._T, w, band)
        self._vertices, self._faces, self._normals = pos.cpu().numpy(), None, nrm.cpu().numpy()

    def _canonical_mesh_device(self):
        """The extraction of write_canonical_mesh, left on the device: (verts, faces, normals)."""
        verts, faces, normals, _ = _mesh.marching_cubes(self._T, self._mc_level, 1)
        return verts, faces, normals

    def write_canonical_mesh(self, path, filename):
        """OBJ file of the canonical surface, step 1, degenerate faces dropped.  Fusion (reference core/fusion.py:577-587):
        skimage's default level, index space, `v` / `vn` / `f a b c` (1-based).  FusionDM (core/fusion_dm.py:339-354): level 0,
        world coordinates, `v` / `vn` / `f a//a b//b c//c`.  The stored mesh and the graph are not touched."""
        self._ensure_volumes()
        verts, faces, normals = self._canonical_mesh_device()
        if self.smooth_iters is not None:        # without the voxel-scale ripple (mesh.smooth), normals from the moved faces
            verts, normals = _mesh.smooth_with_normals(verts, faces, self.smooth_iters)
        if self.simplify_cell is not None:       # a coarser file (mesh.simplify)
            verts, faces, normals, _ = _mesh.simplify_with_normals(verts, faces, normals, self.simplify_cell)
        colors = valid = None
        if self._C is not None:                  # vertex colours (not in the reference): the colour volume sampled at the vertices
            rgb, valid = kernels.sample_colors(self._C, verts.double())         # (of a simplified mesh: at the NEW vertices)
            colors, valid = rgb.cpu().numpy(), valid.cpu().numpy()
        self._write_mesh(os.path.join(path, filename), verts.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy(), colors, valid)

    def write_live_frame_mesh(self, path, filename, warpfield_path):
        """Reference core/fusion.py:588-590, core/fusion_dm.py:356-358 ("Process a warp field file and write the live frame mesh";
        an empty stub in both): the canonical mesh warped into the live frame (live_frame_mesh) with the nodes of `warpfield_path`
        (a file of write_warp_field; None / "" = the current `_nodes`), written in write_canonical_mesh's layout.  Returns the
        file path."""
        nodes = _io.read_warp_field(warpfield_path) if warpfield_path else None
        verts, faces, normals = self.live_frame_mesh(nodes)
        fpath = os.path.join(path, filename)
        self._write_mesh(fpath, verts.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy())
        return fpath

    def write_warp_field(self, path, filename):
        """Reference core/fusion.py:571-573, core/fusion_dm.py:334-336: pickle of `_nodes` into <path>/<filename>__<itercounter>.p."""
        return _io.write_warp_field(self._nodes, path, filename, self._itercounter)

    # ------------------------------------------------------------------ deformation graph
    # The reference's FusionDM carries a second copy of the non-rigid methods ("functions below not useful for now",
    # core/fusion_dm.py:366-560): computeSparsity, computef, warp, dq_blend, construct_graph, update_graph -- the same statements
    # as Fusion's up to white space.  Both classes here inherit the one copy below (and the helpers it calls), so FusionDM's call
    # surface is complete; like in the reference they need `_nodes`, `_vertices`, `_normals`, `_neighbor_look_up`, `_radius` and
    # one correspondence per vertex to be set by the caller.
    def node_arrays(self):
        """(pos (N,3), dq (N,8), w (N,), vertex index (N,)) from the `_nodes` 4-tuples."""
        if len(self._nodes) == 0:
            raise ValueError('the deformation graph is empty: fill _nodes first')
        vidx = np.array([int(n[0]) for n in self._nodes], dtype=np.int64)
        pos = np.array([np.asarray(n[1], dtype=np.float64) for n in self._nodes])
        dq = np.array([np.asarray(n[2], dtype=np.float64) for n in self._nodes])
        w = np.array([float(n[3]) for n in self._nodes], dtype=np.float64)
        return pos, dq, w, vidx

    # ---- A5 (single-point helpers)
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

    # ---- A10
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

    # ---- graph maintenance
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
