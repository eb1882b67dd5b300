"""The scenes of the normal-gate tests (tests/test_assoc_normals_cpu.py, tests/test_gpu_assoc_normals.py): samples on a ball of
the bench scene's camera and grid (dynamicfusion_body_amd/scene.py, C1 maps, 64^3), the live ball moved, live normal maps from the
numpy restatement of the depth preprocessing (tests/depth_prep_np.normals_of).  numpy only."""
import numpy as np

import depth_prep_np as DN
from dynamicfusion_body_amd import scene
from oracle import oracle_np as O

RES = 64
H, W, _F, _CX, _CY = scene.CAMERAS["C1"]
K = scene.intrinsics(_F, _CX, _CY)
KINV = np.linalg.inv(K)
SCALE, CENTER, _ = scene.grid_params(RES)
HALF = RES / 2.0
IDENT = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
N_SAMPLES = 4000                                   # not a multiple of the 128-sample tile: the last tile is ragged


def fibonacci_dirs(n):
    i = np.arange(n, dtype=np.float64) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    theta = np.pi * (1 + 5 ** 0.5) * i
    return np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=-1)


class Scene:
    """pos / nrm: N_SAMPLES Fibonacci samples on a ball of radius_m (outward normals -- the TSDF gradient points into free space);
    the live ball moved by `move` voxels; lws / dms / nmaps: the views' extrinsics, depth maps (no invalid pixels, no wall) and
    live normal maps; node_pos / node_w / nbr: n_nodes Fibonacci nodes on the ball and the samples' knn nearest of them."""

    def __init__(self, radius_m, angles, move=(0.0, 0.0, 1.5), n_nodes=16, knn=4, depth_dtype=np.float64):
        self.dirs = fibonacci_dirs(N_SAMPLES)
        self.radius = radius_m / SCALE
        self.pos = self.dirs * self.radius + HALF
        self.nrm = self.dirs.copy()
        self.move = np.asarray(move, dtype=np.float64)
        self.lws = [scene.view_extrinsic(a) for a in angles]
        self.dms = [scene.render_depth(K, lw, H, W, invalid_frac=0.0, sphere_r=radius_m, wall_z=None, sphere_offset=self.move * SCALE,
                                       dtype=depth_dtype) for lw in self.lws]
        self.nmaps = np.stack([DN.normals_of(d, KINV, 0.03, 0.2)[0] for d in self.dms])
        self.node_pos, self.node_w = scene.fibonacci_nodes(n_nodes, RES, radius_vox=self.radius)
        self.knn = knn
        self.nbr = O.knn_bruteforce(self.pos, self.node_pos, knn)
        self.dqs = np.tile(IDENT, (n_nodes, 1))

    def wrong_side(self, corr, valid):
        """Valid samples whose normal has a negative cosine with the live ball's analytic normal at their correspondence."""
        an = corr - (HALF + self.move)
        return valid & ((an * self.nrm).sum(axis=1) < 0)

    def image_error(self, corr, valid):
        """mean |c - the true image of the sample| over the valid samples, voxels."""
        return float(np.linalg.norm(corr - (self.pos + self.move), axis=1)[valid].mean())


def thin(angles=(0,), **kw):
    """A ball of radius 2 voxels: thinner than any useful distance gate."""
    return Scene(0.05, angles, **kw)


def ordinary(angles=(-40, 0, 40), **kw):
    """The bench scene's sphere: radius 20 voxels."""
    return Scene(scene.SPHERE_R, angles, **kw)


def centre_displacement(dq):
    """Where one node DQ (all nodes share the rigid-mode twist) takes the ball's centre, minus the centre."""
    c = np.asarray(O.dqb_warp(np.asarray(dq, dtype=np.float64), np.array([[HALF, HALF, HALF]])), dtype=np.float64)
    return c[0] - HALF
