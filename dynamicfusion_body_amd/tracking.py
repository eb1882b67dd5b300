"""Camera tracking, KinectFusion's pose estimation: dense projective point-to-plane ICP of a frame's depth and normal maps against
the model's predicted maps, coarse to fine (kernels.depth_halve, kernels.icp_track; semantics in include/dfusion_hip.h).

A CameraTracker holds the schedule; track() takes the frame's depth maps, the cameras they are believed to come from and a
function that predicts the model's maps for given cameras (a ray cast of a volume, a rendered mesh), and returns the cameras the
maps fit best.  Views are tracked independently.  FusionDM.track_frame and SlabFrame.step(track=True) are its callers in this
package; nothing uses it unless asked to."""
import numpy as np
import torch

from . import kernels
from .depth_prep import DepthPrep


def level_intrinsics(K):
    """The intrinsics of the next coarser pyramid level: a pixel's coordinate is its integer index, and pixel (y, x) of the coarse
    map covers the fine pixels 2x, 2x + 1, whose centre lies at 2x + 0.5."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    out = np.array(K, dtype=np.float64)
    out[0, 0], out[0, 1], out[1, 1] = K[0, 0] / 2, K[0, 1] / 2, K[1, 1] / 2
    out[0, 2], out[1, 2] = (K[0, 2] - 0.5) / 2, (K[1, 2] - 0.5) / 2
    return out


def invert_rigid(T):
    """[R^T | -R^T t] of a 3 x 4 [R | t]."""
    T = np.asarray(T, dtype=np.float64).reshape(3, 4)
    return np.concatenate([T[:, :3].T, -(T[:, :3].T @ T[:, 3:])], axis=1)


def project_so3(R):
    """The rotation nearest to R (its polar factor, determinant +1)."""
    u, _, vt = np.linalg.svd(np.asarray(R, dtype=np.float64))
    d = np.sign(np.linalg.det(u @ vt))
    return u @ np.diag([1.0, 1.0, d]) @ vt


def compose(A, B):
    """A B of two 3 x 4 rigid matrices."""
    A = np.asarray(A, dtype=np.float64).reshape(3, 4)
    B = np.asarray(B, dtype=np.float64).reshape(3, 4)
    return np.concatenate([A[:, :3] @ B[:, :3], A[:, :3] @ B[:, 3:] + A[:, 3:]], axis=1)


class CameraTracker:
    """The schedule of a coarse-to-fine frame-to-model ICP.

    K                  : the depth maps' intrinsics (3 x 3) at the finest level
    levels             : pyramid levels (level 0 = the maps as given, each further one halved)
    iters, max_dist,
    normal_cos         : per level, FINEST FIRST: iterations, the gate on the distance between a live point and the model point it
                         projects onto (the maps' units; 0 = none), the smallest cosine between their normals
    huber              : the Huber threshold on the point-to-plane residual (0 = none)
    max_jump           : the largest depth step between neighbours of the finest level that a pyramid tap is averaged across and a
                         normal is computed across; doubled per level
    lm_rel, min_count,
    max_rot, max_trans : the solve's damping and the guards of one step (dfh_icp_track)
    depth_prep         : a DepthPrep that cleans the finest level first, or None"""

    def __init__(self, K, levels=3, iters=(4, 5, 10), max_dist=(0.1, 0.2, 0.4), normal_cos=(0.8, 0.65, 0.5), huber=0.0, depth_prep=None,
                 max_jump=0.05, lm_rel=1e-3, min_count=100, max_rot=0.5, max_trans=0.5, gate_normals=True):
        self.K = np.asarray(K, dtype=np.float64).reshape(3, 3)
        self.levels = int(levels)
        if self.levels < 1:
            raise ValueError("levels must be >= 1, got %d" % self.levels)

        def per_level(name, v):
            v = tuple(v) if isinstance(v, (tuple, list)) else (v,) * self.levels
            if len(v) != self.levels:
                raise ValueError("%s needs one entry per level (%d), finest first, got %d" % (name, self.levels, len(v)))
            return v
        self.iters = tuple(int(i) for i in per_level("iters", iters))
        self.max_dist = tuple(float(x) for x in per_level("max_dist", max_dist))
        self.normal_cos = tuple(float(x) for x in per_level("normal_cos", normal_cos))
        if any(not 0 <= i <= 64 for i in self.iters):
            raise ValueError("iters must lie in 0..64")
        self.huber, self.max_jump, self.lm_rel = float(huber), float(max_jump), float(lm_rel)
        self.min_count, self.max_rot, self.max_trans = int(min_count), float(max_rot), float(max_trans)
        self.depth_prep = depth_prep
        self.gate_normals = bool(gate_normals)
        self.Ks = [self.K]
        for _ in range(1, self.levels):
            self.Ks.append(level_intrinsics(self.Ks[-1]))
        self._tables = {}
        self._scratch = {}

    def _normal_tables(self, device):
        t = self._tables.get(device)
        if t is None:
            t = self._tables[device] = kernels.depth_prep_tables(0, 1.0, 1.0, n_lut=1, device=device)
        return t

    def live_pyramid(self, depths):
        """[(depth (V, H_l, W_l) float32, normals (V, H_l, W_l, 3) float32)] per level, finest first."""
        depths = DepthPrep._to_device(list(depths))
        dev = depths[0].device
        if self.depth_prep is not None:
            depths, _ = self.depth_prep(depths, np.linalg.inv(self.Ks[0]), want_normals=False)
        out = []
        maps = depths
        for l in range(self.levels):
            if l > 0:
                half = kernels.depth_halve(maps, self.max_jump * 2.0 ** (l - 1))
                maps = [half[v] for v in range(half.shape[0])]
            clean, normals = kernels.depth_prep(maps, np.linalg.inv(self.Ks[l]), self._normal_tables(dev), self.max_jump * 2.0 ** l, 0.0,
                                                mask=False)
            out.append((clean, normals))
        return out

    def track(self, depths, lws_prev, model_fn, gate_normals=None):
        """depths: the frame's depth maps (at most 16 (H, W) maps of one shape; CUDA tensors, or numpy arrays that are uploaded);
        lws_prev: one world -> camera 3 x 4 per map, the prior; model_fn(lws_prev, K_l, H_l, W_l) -> (depth (V, H_l, W_l),
        normals (V, H_l, W_l, 3)), float32 CUDA: the model as the cameras lws_prev see it through K_l, called once per level.
        gate_normals: this call's choice instead of the constructor's (False: the model's normals do not face the camera).
        Returns (lws, stats): lws[v] = T_v^-1 lws_prev[v], T_v the live camera -> model camera motion the ICP found (its rotation
        projected onto SO(3)); a view whose last iteration at the finest level was refused is lost and keeps lws_prev[v].
        stats: {"lost": (V,) bool, "T": (V, 3, 4), "levels": [per level, finest first, the (V, iters, 40) records]}.  The levels'
        launches are queued back to back; the poses are read back once, at the end."""
        depths = list(depths)
        lws_prev = [np.asarray(l, dtype=np.float64).reshape(3, 4) for l in lws_prev]
        V = len(depths)
        if V == 0 or V > 16:
            raise ValueError("track takes 1..16 depth maps, got %d" % V)
        if len(lws_prev) != V:
            raise ValueError("one camera per depth map: %d cameras for %d maps" % (len(lws_prev), V))
        gate = self.gate_normals if gate_normals is None else bool(gate_normals)
        pyr = self.live_pyramid(depths)
        dev = pyr[0][0].device
        scratch = self._scratch.get((dev, V))
        if scratch is None:
            scratch = self._scratch[(dev, V)] = kernels.icp_track_scratch(V, dev)
        T = torch.eye(4, dtype=torch.float64)[:3].repeat(V, 1, 1).to(dev).contiguous()
        records = [None] * self.levels
        for l in range(self.levels - 1, -1, -1):
            live_d, live_n = pyr[l]
            H, W = int(live_d.shape[1]), int(live_d.shape[2])
            model_d, model_n = model_fn(lws_prev, self.Ks[l], H, W)
            records[l], _ = kernels.icp_track(live_d, live_n if gate else None, model_d.contiguous(), model_n.contiguous(),
                                              self.Ks[l], np.linalg.inv(self.Ks[l]), T, self.iters[l], max_dist=self.max_dist[l],
                                              min_cos=self.normal_cos[l], huber=self.huber, lm_rel=self.lm_rel, min_count=self.min_count,
                                              max_rot=self.max_rot, max_trans=self.max_trans, scratch=scratch)
        Th = T.cpu().numpy()
        records = [r.cpu().numpy() for r in records]
        fine = next((r for r in records if r.shape[1] > 0), None)
        lost = np.zeros(V, dtype=bool) if fine is None else fine[:, -1, 29] == 0.0
        lws = []
        for v in range(V):
            if lost[v]:
                lws.append(lws_prev[v].copy())
                continue
            Tv = np.concatenate([project_so3(Th[v, :, :3]), Th[v, :, 3:]], axis=1)
            lws.append(compose(invert_rigid(Tv), lws_prev[v]))
        return lws, {"lost": lost, "T": Th, "levels": records}
