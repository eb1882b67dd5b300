"""Rendered-view descriptors (K15): the reference's compute_correspondence (core/sdf.py:95-150) around a per-pixel feature
network that stays the caller's.

    fusion.descriptor_fn = PooledDescriptors(feature_fn)

`feature_fn` maps the (V, H, W) uint8 depth images of the views to (V, H, W, D) float32 per-pixel features; everything else --
the mesh normalisation, the ring of cameras, the vertex-id render, the depth-to-image expression and the pooling of the
features onto the vertices -- runs here, the render and the pooling on the device (dfh_render_vertex_ids, dfh_pool_features)."""
import numpy as np
import torch

from . import _lib, mesh
from .device import current_stream_ptr, require_gpu


def regularize_mesh(vertices, flipyz=False):
    """core/meshutil.py:62-69 in fp64 on a copy: the mesh centred on its mean and scaled to a height (y extent) of 1.8.
    flipyz swaps the y and z columns first (the reference's tuple assignment on two views of one array leaves z in both
    columns, and in the caller's array; a real swap of a copy is what is done here)."""
    v = np.array(vertices, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 3 or len(v) == 0:
        raise ValueError("vertices must be (n,3) with n > 0, got shape %s" % (np.shape(vertices),))
    if flipyz:
        v = v[:, [0, 2, 1]]
    scale = 1.8 / (np.max(v[:, 1]) - np.min(v[:, 1]))
    transform = -np.mean(v, 0)
    return (v + transform) * scale


def _rotate(m, angle, axis):
    """GLM's rotate as the reference evaluates it (core/gl/glm.py): the 3x3 block in fp64 stored as float32, the product with
    `m` in float32, every column summed left to right."""
    c, s = np.cos(angle), np.sin(angle)
    ax = np.asarray(axis, dtype=np.float32)
    n = np.linalg.norm(ax)
    ax = ax if n == 0 else ax / n
    a = ax.astype(np.float64)
    t = (1 - c) * a
    rot = np.array([[c + t[0] * a[0], t[0] * a[1] + s * a[2], t[0] * a[2] - s * a[1]],
                    [t[1] * a[0] - s * a[2], c + t[1] * a[1], t[1] * a[2] + s * a[0]],
                    [t[2] * a[0] + s * a[1], t[2] * a[1] - s * a[0], c + t[2] * a[2]]]).astype(np.float32)
    res = np.zeros((4, 4), dtype=np.float32)
    for j in range(3):
        res[:, j] = m[:, 0] * rot[j][0] + m[:, 1] * rot[j][1] + m[:, 2] * rot[j][2]
    res[:, 3] = m[:, 3]
    return res


def _translate(m, v):
    v = np.asarray(v, dtype=np.float32)
    res = m.copy()
    res[:, 3] = m[:, 0] * v[0] + m[:, 1] * v[1] + m[:, 2] * v[2] + m[:, 3]
    return res


def turntable_views(width=512, height=512, znear=1.0, zfar=3.5, max_swi=70, fov_deg=70, swi=35, dis=200, step_deg=15):
    """The reference's cameras (core/sdf.py:108-131: a swing of swi - max_swi / 2 degrees, `dis` / 100 back along z, a turn
    of 0, step_deg, ... < 360 degrees about y, a GL perspective of fov_deg) for mesh.render / mesh.render_vertex_ids:
    (K (3,3), lws (V,3,4)) such that a point with GL normalised device coordinates (nx, ny) and clip w lands at
    u = (W - 1) / 2 - (W / 2) nx, v = (H - 1) / 2 - (H / 2) ny (the reference flips both axes of what it reads back) with
    camera depth w.  The matrices are built in float32 step by step as the reference builds them, so the views agree with its
    `mvp` to fp64 rounding; the rows of lws are the clip-space x, y and w rows (the focal length sits in them, K only scales by
    half the image size), so lws is affine, not rigid.  znear / zfar do not enter the three rows used."""
    del znear, zfar
    tan_half = np.tan(np.radians(fov_deg) / 2)
    p00 = np.float32(1 / (1.0 * tan_half))
    p11 = np.float32(1 / tan_half)
    lws = []
    for rot in range(0, 360, int(step_deg)):
        mod = np.identity(4, dtype=np.float32)
        mod = _rotate(mod, np.radians(swi - max_swi / 2), (0, 1, 0))
        mod = _translate(mod, (0, 0, -dis / 100.0))
        mod = _rotate(mod, np.radians(rot), (0, 1, 0))
        lws.append(np.stack([p00 * mod[0], p11 * mod[1], -mod[2]]).astype(np.float64))
    K = np.array([[-width / 2.0, 0.0, (width - 1) / 2.0], [0.0, -height / 2.0, (height - 1) / 2.0], [0.0, 0.0, 1.0]])
    return K, np.stack(lws)


def _device_tensor(a, dtype, dev):
    """numpy array or tensor -> contiguous tensor of `dtype` on `dev`; a device tensor that already is one is used in place."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dtype).contiguous()


def pool_features(vid, feats, n_verts):
    """dfh_pool_features (csrc/dfh_pool.hip, semantics in include/dfusion_hip.h): the mean of the feature rows of every
    vertex's pixels, summed in float32 in ascending pixel order -- bit-identical from run to run.  vid: any shape, integer,
    values outside [0, n_verts) = no vertex; feats: that shape + (D,), D <= 64.  numpy arrays or CUDA tensors (int32 /
    float32 contiguous device tensors are used in place).  Returns (feat (n_verts, D) float32, cnt (n_verts,) int32) as CUDA
    tensors."""
    require_gpu()
    lib = _lib.load()
    n_verts = int(n_verts)
    if n_verts < 0:
        raise ValueError("n_verts must be >= 0, got %d" % n_verts)
    if feats.ndim != vid.ndim + 1 or tuple(feats.shape[:-1]) != tuple(vid.shape):
        raise ValueError("feats must have the shape of vid plus (D,): vid %s, feats %s" % (tuple(vid.shape), tuple(feats.shape)))
    dim = int(feats.shape[-1])
    if not 1 <= dim <= 64:
        raise ValueError("1 to 64 channels are supported, got %d" % dim)
    dev = torch.device("cuda", torch.cuda.current_device())
    ids = _device_tensor(vid, torch.int32, dev)
    F = _device_tensor(feats, torch.float32, dev)
    n_pixels = ids.numel()
    out = torch.empty((n_verts, dim), dtype=torch.float32, device=dev)
    cnt = torch.empty((n_verts,), dtype=torch.int32, device=dev)
    nbytes = lib.dfh_pool_features_workspace_bytes(n_pixels, n_verts)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    _lib.check(lib.dfh_pool_features(ids.data_ptr(), F.data_ptr(), n_pixels, dim, n_verts, out.data_ptr(), cnt.data_ptr(), ws.data_ptr(),
                                     nbytes, current_stream_ptr()), "dfh_pool_features")
    return out, cnt


class PooledDescriptors:
    """A callable (vertices (n,3), faces (m,3)) -> (n, D) float32 numpy, usable as Fusion.descriptor_fn: the mesh regularised
    (regularize_mesh), rendered from turntable_views(**view_options) with a vertex id in every pixel, `feature_fn` called ONCE
    with the (V, H, W) uint8 CUDA tensor of depth images, its (V, H, W, D) float32 result (CUDA tensor or numpy) pooled onto the
    vertices.  A vertex no view shows gets zeros; `last_count` holds the pixels per vertex of the last call (CUDA int32).
    view_options: the arguments of turntable_views, and flipyz."""

    def __init__(self, feature_fn, flipyz=False, **view_options):
        if not callable(feature_fn):
            raise ValueError("feature_fn must be callable")
        self.feature_fn = feature_fn
        self.flipyz = bool(flipyz)
        self.width = int(view_options.get("width", 512))
        self.height = int(view_options.get("height", 512))
        self.znear = float(view_options.get("znear", 1.0))
        self.zfar = float(view_options.get("zfar", 3.5))
        self.K, self.lws = turntable_views(**view_options)
        self.last_count = None

    def __call__(self, vertices, faces):
        if faces is None:
            raise ValueError("rendered-view descriptors need the mesh's faces (a pruned vertex set has none)")
        reg = regularize_mesh(vertices, self.flipyz)
        vid, image = mesh.render_vertex_ids(reg, faces, self.K, self.lws, self.height, self.width, self.znear, self.zfar)
        feats = self.feature_fn(image)
        if feats.ndim != 4 or tuple(feats.shape[:3]) != tuple(image.shape):
            raise ValueError("feature_fn must return (V, H, W, D) features for the %s images, got shape %s"
                             % (tuple(image.shape), tuple(feats.shape)))
        out, cnt = pool_features(vid, feats, len(reg))
        self.last_count = cnt
        return out.cpu().numpy()
