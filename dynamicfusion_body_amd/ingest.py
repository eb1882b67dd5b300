"""RGB-D ingest, the stage in front of everything else: what a sensor delivers -- uint16 depth maps in device units through a
distorted lens with per-camera intrinsics, and the images of a second, colour camera beside each depth camera -- becomes what the
rest of the package reads: undistorted depth maps through ONE pinhole `K` (negative depth, 0 = no measurement), colour registered
to the depth pixels with an occlusion test (RGBX, X = 255 where the colour is valid) and depth maps that keep only the pixels
with a colour, for the colour fusion.  At most three kernel launches for all views of a frame (kernels.rgbd_ingest,
dfh_rgbd_ingest; the semantics are in include/dfusion_hip.h).

Nothing uses it unless asked to: SlabFrame(ingest=...), FusionDM.ingest and Fusion.ingest put an RGBDIngest in front of the
methods that sweep a list of maps.  Colour-invalid pixels reach the photometric term as RGB 0: that is what its `photo_max_diff`
gate is for."""
import ctypes

import numpy as np
import torch

from . import _lib, kernels
from .device import require_gpu

DEFAULT_OCCL_TOL = 0.05      # in the units of z = raw * depth_scale (metres at the default scale).  Chosen on the sphere-and-wall
                             # scene of tests/test_ingest.py (recorded in tests/golden/ingest_occlusion.json): the count of correctly
                             # coloured pixels the test drops has levelled off there (108 of 18 692; 349 at 0.02, 103 at 0.1) and no
                             # wall pixel takes the sphere's colour (102 without the test)


class RGBDCalibration:
    """One view's calibration: the raw depth camera (intrinsics fd = (fx, fy, cx, cy), distortion kd = (k1, k2, p1, p2, k3) in
    OpenCV's Brown-Conrady order), the colour camera (fc, kc) and T_dc, the 3 x 4 (or 4 x 4) transform from the depth camera's frame
    to the colour camera's in the units of z = raw * depth_scale.  A depth-only rig leaves the colour side at its defaults."""

    def __init__(self, depth_intrinsics, depth_distortion=None, color_intrinsics=None, color_distortion=None, T_dc=None):
        def vec(a, n, default):
            a = np.asarray(default if a is None else a, dtype=np.float64).reshape(-1)
            if a.size != n:
                raise ValueError("expected %d values, got %d" % (n, a.size))
            return a
        self.fd = vec(depth_intrinsics, 4, None)
        self.kd = vec(depth_distortion, 5, np.zeros(5))
        self.fc = vec(color_intrinsics, 4, self.fd)
        self.kc = vec(color_distortion, 5, np.zeros(5))
        T = np.eye(4)[:3] if T_dc is None else np.asarray(T_dc, dtype=np.float64)
        if T.shape == (4, 4):
            T = T[:3]
        if T.size != 12:
            raise ValueError("T_dc must be 3 x 4 (or its 12 numbers, row-major) or 4 x 4")
        T = T.reshape(3, 4)
        self.T_dc = np.ascontiguousarray(T)
        if not all(np.isfinite(a).all() for a in (self.fd, self.kd, self.fc, self.kc, self.T_dc)):
            raise ValueError("calibration values must be finite")
        if not (self.fd[0] > 0 and self.fd[1] > 0 and self.fc[0] > 0 and self.fc[1] > 0):
            raise ValueError("focal lengths must be > 0")

    def record(self):
        """The 30 numbers of a dfh_rgbd_view."""
        return np.concatenate([self.fd, self.kd, self.fc, self.kc, self.T_dc.reshape(-1)])


class RGBDIngest:
    """The stage's parameters.

    calibs        : one RGBDCalibration per view, in the order the frames' maps come in
    depth_size    : (Hd, Wd) of the raw depth maps -- and of every output
    color_size    : (Hc, Wc) of the raw colour images (None: a depth-only rig)
    out_intrinsics: (fx, fy, cx, cy) of the ideal pinhole every output map is resampled to; `K` / `Kinv` are its 3 x 3 forms, the
                    ones to give the rest of the pipeline
    depth_scale   : z = raw * depth_scale (1e-3: millimetres to metres)
    z_range       : (z_min, z_max) a measurement must lie in; z_max <= 0: no upper bound
    occl_tol      : how far behind the colour camera's z-buffer a pixel may lie and still take a colour (the units of z)
    sample        : "bilinear" or "nearest" colour lookup
    max_splat     : bound (1..16) on the columns and rows of the z-buffer one depth pixel covers; it must not be smaller than
                    the ratio of the colour image's pixel pitch to the depth image's, or background shows through the gaps"""

    def __init__(self, calibs, depth_size, color_size, out_intrinsics, depth_scale=1e-3, z_range=(0.0, 0.0), occl_tol=DEFAULT_OCCL_TOL,
                 sample="bilinear", max_splat=8):
        self.calibs = list(calibs)
        if not self.calibs or not all(isinstance(c, RGBDCalibration) for c in self.calibs):
            raise ValueError("calibs must be a non-empty list of RGBDCalibration")
        self.depth_size = tuple(int(n) for n in depth_size)
        self.color_size = None if color_size is None else tuple(int(n) for n in color_size)
        k = np.asarray(out_intrinsics, dtype=np.float64).reshape(-1)
        if k.size != 4 or not np.isfinite(k).all() or not (k[0] > 0 and k[1] > 0):
            raise ValueError("out_intrinsics must be finite (fx, fy, cx, cy) with fx, fy > 0")
        self.out_intrinsics = k
        self.K = np.array([[k[0], 0.0, k[2]], [0.0, k[1], k[3]], [0.0, 0.0, 1.0]])
        self.Kinv = np.linalg.inv(self.K)
        self.depth_scale = float(depth_scale)
        self.z_min, self.z_max = (float(z) for z in z_range)
        self.occl_tol = float(occl_tol)
        self.max_splat = int(max_splat)
        self.sample = sample
        if not self.depth_scale > 0.0 or not np.isfinite(self.depth_scale):
            raise ValueError("depth_scale must be finite and > 0")
        if not self.occl_tol >= 0.0:
            raise ValueError("occl_tol must be >= 0")
        if not 1 <= self.max_splat <= 16:
            raise ValueError("max_splat must be 1..16, got %d" % self.max_splat)
        if sample not in kernels.RGBD_SAMPLE:
            raise ValueError("sample must be one of %s, not %r" % (sorted(kernels.RGBD_SAMPLE), sample))
        self._ws = {}                             # (device, views of the chunk) -> workspace, reused from frame to frame
        self._records = []                        # per chunk of 16 views: the calibration as the library's records, packed once
        for i in range(0, len(self.calibs), 16):
            chunk = self.calibs[i:i + 16]
            recs = (_lib.RGBDView * len(chunk))()
            for r, c in zip(recs, chunk):
                ctypes.memmove(ctypes.byref(r), np.ascontiguousarray(c.record()).ctypes.data, 240)
            self._records.append(recs)

    @staticmethod
    def _upload(a, bits16):
        """A raw map or image on the device.  numpy uint16 travels as int16 (the same bits: kernels.rgbd_ingest takes either)."""
        if isinstance(a, torch.Tensor):
            return a.contiguous() if a.is_cuda else a.contiguous().cuda()
        a = np.ascontiguousarray(a)
        if bits16:
            if a.dtype != np.uint16:
                raise ValueError("a raw depth map must be uint16, got %s" % a.dtype)
            a = a.view(np.int16)
        return torch.from_numpy(a).cuda()

    def __call__(self, raw_depths, raw_colors=None, out=None):
        """raw_depths: one (Hd, Wd) uint16 map per calibrated view (numpy arrays are uploaded); raw_colors: None, or one
        (Hc, Wc, 3) / (Hc, Wc, 4) uint8 image per view.  Returns (depths (V, Hd, Wd) float32, colors (V, Hd, Wd, 4) uint8 or None,
        color_depths (V, Hd, Wd) float32 or None).  out=(depths, colors, color_depths): buffers to write into.  More than 16 views
        are taken 16 at a time."""
        raw_depths = list(raw_depths)
        V = len(raw_depths)
        if V != len(self.calibs):
            raise ValueError("%d raw depth maps for %d calibrated views" % (V, len(self.calibs)))
        colour = raw_colors is not None
        if colour:
            raw_colors = list(raw_colors)
            if len(raw_colors) != V:
                raise ValueError("one colour image per depth map: %d images for %d maps" % (len(raw_colors), V))
            if self.color_size is None:
                raise ValueError("colour images for a rig calibrated without a colour camera (color_size=None)")
        for d in raw_depths:
            if tuple(d.shape) != self.depth_size:
                raise ValueError("raw depth map of %s pixels, calibrated for %s" % (tuple(d.shape), self.depth_size))
        if colour:
            for c in raw_colors:
                if tuple(c.shape[:2]) != self.color_size:
                    raise ValueError("raw colour image of %s pixels, calibrated for %s" % (tuple(c.shape[:2]), self.color_size))
        require_gpu()
        ds = [self._upload(d, True) for d in raw_depths]
        cs = [self._upload(c, False) for c in raw_colors] if colour else None
        dev = ds[0].device
        Hd, Wd = self.depth_size
        if out is None:
            out = (torch.empty((V, Hd, Wd), dtype=torch.float32, device=dev),
                   torch.empty((V, Hd, Wd, 4), dtype=torch.uint8, device=dev) if colour else None,
                   torch.empty((V, Hd, Wd), dtype=torch.float32, device=dev) if colour else None)
        depths, colors, cdepths = out
        if depths is None or tuple(depths.shape) != (V, Hd, Wd) or (colour and (colors is None or tuple(colors.shape) != (V, Hd, Wd, 4))) \
                or (cdepths is not None and tuple(cdepths.shape) != (V, Hd, Wd)):
            raise ValueError("out must be (depths (V, Hd, Wd), colors (V, Hd, Wd, 4), color_depths (V, Hd, Wd) or None) for these %d views" % V)
        for i in range(0, V, 16):                                    # (a call takes at most 16 views)
            n = min(16, V - i)
            ws = None
            if colour:
                ws = self._ws.get((dev, n))
                if ws is None:
                    ws = self._ws[(dev, n)] = kernels.rgbd_ingest_workspace(n, self.color_size[0], self.color_size[1], dev)
            kernels.rgbd_ingest(ds[i:i + n], cs[i:i + n] if colour else None, self._records[i // 16],
                                self.out_intrinsics, self.depth_scale, self.z_min, self.z_max, self.occl_tol, self.max_splat, self.sample,
                                out=(depths[i:i + n], colors[i:i + n] if colour else None,
                                     cdepths[i:i + n] if colour and cdepths is not None else None), workspace=ws)
        if not colour:
            return depths, None, None
        return depths, colors, cdepths

    def frame(self, raw_depths, raw_colors=None, K=None):
        """__call__ for the hooks: per-view lists (depth maps, registered colour images or None, colour-only depth maps or
        None).  K: the caller's intrinsics, which must be the pinhole this stage resamples to."""
        if K is not None and not np.array_equal(np.asarray(K, dtype=np.float64), self.K):
            raise ValueError("the camera matrix must equal ingest.K: the stage resamples every depth map to that pinhole")
        d, c, cd = self(raw_depths, raw_colors)
        V = d.shape[0]
        return [d[v] for v in range(V)], None if c is None else [c[v] for v in range(V)], None if cd is None else [cd[v] for v in range(V)]
