"""Depth preprocessing, the first stage of the KinectFusion / DynamicFusion frame: bilateral smoothing of the raw depth maps, a
live normal map, and removal of the pixels no normal can be computed for (depth discontinuities -- "flying pixels" --, isolated
pixels, grazing angles).  One kernel launch for all views of a frame (kernels.depth_prep, dfh_depth_prep).

The cleaned maps keep the convention every other entry point reads (negative depth, 0 = no measurement), so a DepthPrep can be
put in front of anything that takes depth maps: FusionDM.depth_prep / Fusion.depth_prep / SlabFrame(depth_prep=...) do so for
the methods that sweep a list of maps.  Nothing uses it unless asked to."""
import torch

from . import kernels
from .device import depths_to_device


class DepthPrep:
    """The stage's parameters and its filter tables (built once per device).

    radius, sigma_s : window half-size and spatial sigma of the bilateral filter, in pixels (radius 0: no smoothing)
    sigma_r         : range sigma, in the depth maps' units (metres for scene.py); neighbours further than cut * sigma_r from the
                      centre in depth do not take part
    max_jump        : largest depth step to a 4-neighbour across which a normal is still computed (the maps' units)
    min_cos         : smallest cosine between the normal and the viewing ray (0 keeps every angle)
    mask            : True = pixels without a normal are removed from the cleaned maps
    n_lut, cut      : size and reach of the range-weight table (kernels.depth_prep_tables)"""

    def __init__(self, radius=3, sigma_s=1.5, sigma_r=0.01, max_jump=0.03, min_cos=0.2, mask=True, n_lut=1024, cut=3.0):
        self.radius, self.sigma_s, self.sigma_r = int(radius), float(sigma_s), float(sigma_r)
        self.max_jump, self.min_cos, self.mask = float(max_jump), float(min_cos), bool(mask)
        self.n_lut, self.cut = int(n_lut), float(cut)
        if not 0.0 <= self.min_cos <= 1.0:
            raise ValueError("min_cos must lie in [0, 1]")
        if not self.max_jump >= 0.0:
            raise ValueError("max_jump must be >= 0")
        kernels.depth_prep_tables(self.radius, self.sigma_s, self.sigma_r, self.n_lut, self.cut, device="cpu")   # (argument checks)
        self._tables = {}

    def tables(self, device):
        """(spatial, range_lut, range_scale) on `device`, computed on first use."""
        device = torch.device(device)
        t = self._tables.get(device)
        if t is None:
            t = self._tables[device] = kernels.depth_prep_tables(self.radius, self.sigma_s, self.sigma_r, self.n_lut, self.cut,
                                                                 device=device)
        return t

    @staticmethod
    def _to_device(depths):
        """fuseDepths' dtype rule for a list (device.depths_to_device)."""
        return depths_to_device(depths)

    def __call__(self, depths, Kinv, want_normals=True, out=None):
        """depths: list of (H, W) maps of one shape (CUDA tensors, or numpy arrays that are uploaded); Kinv: inverse intrinsics.
        Returns (list of V contiguous (H, W) float32 views of the cleaned maps, normals (V, H, W, 3) float32 or None).
        out=(clean (V, H, W), normals (V, H, W, 3) or None): buffers to write into instead of fresh tensors."""
        depths = self._to_device(list(depths))
        V = len(depths)
        if V == 0:
            return [], None
        H, W = depths[0].shape
        dev = depths[0].device
        if out is None:
            out = (torch.empty((V, H, W), dtype=torch.float32, device=dev),
                   torch.empty((V, H, W, 3), dtype=torch.float32, device=dev) if want_normals else None)
        clean, normals = out
        if clean is None or tuple(clean.shape) != (V, H, W) or (normals is not None and tuple(normals.shape) != (V, H, W, 3)):
            raise ValueError("out must be (clean (V, H, W), normals (V, H, W, 3) or None) for these %d maps" % V)
        for i in range(0, V, 16):                                  # (a launch takes at most 16 maps)
            kernels.depth_prep(depths[i:i + 16], Kinv, self.tables(dev), self.max_jump, self.min_cos, mask=self.mask,
                               out=(clean[i:i + 16], None if normals is None else normals[i:i + 16]))
        return [clean[v] for v in range(V)], normals
