"""Mesh extraction and the canonical-mesh file: the reference's `marching_cubes` /
`write_canonical_mesh` (core/fusion_dm.py:319-331,339-354, core/fusion.py:554-568).

`marching_cubes` runs the HIP kernels of csrc/dfh_mesh.hip (count -> scan -> vertices -> faces) and
has skimage's call shape: (verts, faces, normals, values), with `level=None` meaning
(min + max) / 2 (skimage's documented default, which is what the reference's `marching_cubes()`
gets since it passes no level)."""
import ctypes

import numpy as np
import torch

from . import _lib
from .device import HostScalar, current_stream_ptr, dtype_code, require_gpu, torch_dtype


def marching_cubes(volume, level=None, step_size=1, as_numpy=False, order="reference", visit_all_tiles=False):
    """volume: 3-D CUDA tensor (fp32 / fp64, contiguous).  Returns verts (V,3) fp32 in array-index
    coordinates, faces (F,3) int32, unit normals (V,3) fp32 pointing down the gradient, values (V,)
    fp32 -- CUDA tensors, or numpy arrays with as_numpy=True.  Zero-area faces are not emitted
    (allow_degenerate=False, the only mode the reference uses for its outputs).
    order="reference": skimage's numbering (faces cube by cube, vertices by first use, unused vertices
    dropped); order="lattice": vertices by owning lattice point (skips the renumbering pass).
    visit_all_tiles: emit passes over every tile instead of the compacted list (same result; for tests)."""
    return marching_cubes_begin(volume, level, step_size).finish(as_numpy=as_numpy, order=order, visit_all_tiles=visit_all_tiles)


class marching_cubes_begin:
    """marching_cubes in two halves: the constructor launches the count pass (on the current stream) and returns; finish() waits
    for the totals, launches the emit passes and returns the mesh.  A caller with other work to queue in between (a frame loop
    that has just updated the canonical volume) starts the count early and collects the mesh later.
    Ordering: the count pass's stream is remembered and an event is recorded behind it; finish() may run on any stream -- it
    makes that stream wait for the event before the emit passes read the count pass's workspace.  The volume must not change
    between the two halves (the totals that size the outputs were counted on it): finish() checks the volume tensor's
    version counter and refuses a volume that was written through torch in between (a write through the C ABI is the caller's
    responsibility)."""

    def __init__(self, volume, level=None, step_size=1):
        require_gpu()
        self.lib = lib = _lib.load()
        if not (isinstance(volume, torch.Tensor) and volume.is_cuda and volume.dim() == 3 and volume.is_contiguous()):
            raise ValueError("volume must be a contiguous 3-D CUDA tensor")
        step = int(step_size)
        if step < 1:
            raise ValueError("step_size must be at least 1")                         # skimage raises ValueError too
        if min(volume.shape) < 2:
            raise ValueError("Input array must be at least 2x2x2.")
        if level is None:
            level = 0.5 * (float(volume.min()) + float(volume.max()))
        self.volume, self.step, self.level = volume, step, float(level)
        self.res = _lib.iarr(volume.shape)
        nbytes = lib.dfh_mc_workspace_bytes(self.res, step)
        self.ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=volume.device)
        self.totals = HostScalar(torch.int64, 3)      # (vertices, faces, active tiles: stored into pinned host memory by the scan)
        _lib.check(lib.dfh_mc_count(volume.data_ptr(), dtype_code(volume), self.res, step, self.level, self.ws.data_ptr(),
                                    self.ws.numel() * 8, self.totals.ptr(), current_stream_ptr()), "dfh_mc_count")
        self._count_stream = current_stream_ptr()
        self._counted = torch.cuda.Event()
        self._counted.record()
        self._version = volume._version

    def finish(self, as_numpy=False, order="reference", visit_all_tiles=False):
        if order not in ("reference", "lattice"):
            raise ValueError("order must be 'reference' or 'lattice'")
        lib, volume, ws = self.lib, self.volume, self.ws
        if volume._version != self._version:
            raise RuntimeError("the volume was modified between marching_cubes_begin() and finish(): the counted totals no longer "
                               "describe it")
        if current_stream_ptr() != self._count_stream:
            torch.cuda.current_stream().wait_event(self._counted)       # the emit passes read the count pass's workspace
        nv, nf, nactive = self.totals.get()
        if nv >= (1 << 29) or nf >= (1 << 31) // 3:
            raise ValueError("surface too large for 32-bit mesh indices (%d vertices, %d faces)" % (nv, nf))
        dev = volume.device
        verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        values = torch.empty((nv,), dtype=torch.float32, device=dev)
        faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        _lib.check(lib.dfh_mc_emit(volume.data_ptr(), dtype_code(volume), self.res, self.step, self.level, ws.data_ptr(), ws.numel() * 8,
                                   verts.data_ptr(), normals.data_ptr(), values.data_ptr(), faces.data_ptr(), nv, nf,
                                   -1 if visit_all_tiles else nactive, current_stream_ptr()), "dfh_mc_emit")
        if order == "reference":
            nbytes = lib.dfh_mc_reorder_workspace_bytes(nv, nf)
            ws2 = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
            v2, n2, val2 = torch.empty_like(verts), torch.empty_like(normals), torch.empty_like(values)
            used = HostScalar(torch.int64)
            _lib.check(lib.dfh_mc_reorder(verts.data_ptr(), normals.data_ptr(), values.data_ptr(), faces.data_ptr(), nv, nf,
                                          v2.data_ptr(), n2.data_ptr(), val2.data_ptr(), used.ptr(), ws2.data_ptr(),
                                          ws2.numel() * 8, current_stream_ptr()), "dfh_mc_reorder")
            nu = used.get()
            verts, normals, values = v2[:nu], n2[:nu], val2[:nu]
        if as_numpy:
            return verts.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy(), values.cpu().numpy()
        return verts, faces, normals, values


def obj_colors(colors, valid, n_verts):
    """The r g b columns of an OBJ file's coloured vertex rows: colors ((n, 3), values in [0, 255]) rounded (rint) and clamped to
    a uint8, over 255; rows that are not `valid` ((n,) bool; None: all) or not finite are 0.5 grey."""
    rgb = np.asarray(colors, dtype=np.float64).reshape(-1, 3)
    if len(rgb) != n_verts:
        raise ValueError("%d colours for %d vertices" % (len(rgb), n_verts))
    ok = np.ones(len(rgb), dtype=bool) if valid is None else np.asarray(valid, dtype=bool).reshape(-1)
    ok = ok & np.all(np.isfinite(rgb), axis=1)
    rgb = np.clip(np.rint(np.where(ok[:, None], rgb, 0.0)), 0, 255).astype(np.uint8) / 255.0
    return np.where(ok[:, None], rgb, 0.5)


def write_obj(fpath, verts, faces, normals, ind=None, colors=None, valid=None):
    """The reference's OBJ layout (core/fusion_dm.py:339-354): `v x y z` rows, then `vn`, then
    `f a//a b//b c//c` with 1-based indices, `%f` formatting; `ind` (4x4) maps index space to world
    (`self._IND`: rotation applied to normals, rotation + translation to vertices).
    colors ((n, 3), values in [0, 255]; not in the reference): the vertex rows become `v x y z r g b`, the widespread
    vertex-colour extension, r g b = the value rounded (rint) and clamped to a uint8, over 255.  Vertices that are not `valid`
    ((n,) bool; default: all) are written as 0.5 grey.  Without colours the file is what it always was."""
    verts = np.asarray(verts, dtype=np.float64)
    normals = np.asarray(normals, dtype=np.float64)
    faces = np.asarray(faces)
    if ind is not None:
        ind = np.asarray(ind, dtype=np.float64)
        rot, trans = ind[:3, :3], ind[:3, 3]
        verts = verts @ rot.T + trans
        normals = normals @ rot.T
    with open(fpath, "w") as f:
        if colors is None:
            f.write("".join("v %f %f %f\n" % (v[0], v[1], v[2]) for v in verts))
        else:
            rgb = obj_colors(colors, valid, len(verts))
            f.write("".join("v %f %f %f %f %f %f\n" % (v[0], v[1], v[2], c[0], c[1], c[2]) for v, c in zip(verts, rgb)))
        f.write("".join("vn %f %f %f\n" % (n[0], n[1], n[2]) for n in normals))
        f.write("".join("f %d//%d %d//%d %d//%d\n" % (a + 1, a + 1, b + 1, b + 1, c + 1, c + 1) for a, b, c in faces))


def read_obj(fpath):
    """v / vn / f rows of an OBJ file -> (verts, faces as stored, normals); text parsing only."""
    V, N, F = [], [], []
    with open(fpath) as f:
        for line in f:
            t = line.split()
            if not t:
                continue
            if t[0] == "v":
                V.append([float(x) for x in t[1:4]])
            elif t[0] == "vn":
                N.append([float(x) for x in t[1:4]])
            elif t[0] == "f":
                F.append([int(x.split("/")[0]) for x in t[1:4]])
    return (np.array(V, dtype=np.float64).reshape(-1, 3), np.array(F, dtype=np.int64).reshape(-1, 3),
            np.array(N, dtype=np.float64).reshape(-1, 3))


def read_obj_colors(fpath):
    """The r g b columns of an OBJ file's `v x y z r g b` rows: (n, 3) float64 in [0, 1], or None when the file's vertex rows
    carry no colours; text parsing only."""
    C, plain = [], 0
    with open(fpath) as f:
        for line in f:
            t = line.split()
            if t and t[0] == "v":
                if len(t) >= 7:
                    C.append([float(x) for x in t[4:7]])
                else:
                    plain += 1
    if not C or plain:
        return None
    return np.array(C, dtype=np.float64).reshape(-1, 3)


def _view_table(K, lws):
    """(K rows, lw rows, n_views) as flat fp64 numpy arrays: K one 3x3 (shared) or one per view; lws one 3x4 or a list."""
    lw = np.asarray(lws, dtype=np.float64)
    if lw.ndim == 2:
        lw = lw[None]
    if lw.ndim != 3 or lw.shape[1:] != (3, 4) or len(lw) == 0:
        raise ValueError("lws must be one 3x4 world->camera matrix or a list of them, got shape %s" % (np.shape(lws),))
    Km = np.asarray(K, dtype=np.float64)
    if Km.shape == (3, 3):
        Km = np.broadcast_to(Km, (len(lw), 3, 3))
    if Km.shape != (len(lw), 3, 3):
        raise ValueError("K must be 3x3 (or one 3x3 per view), got shape %s" % (np.shape(K),))
    if not (np.all(Km[:, 1, 0] == 0) and np.all(Km[:, 2, :2] == 0) and np.all(Km[:, 2, 2] == 1)):
        raise ValueError("K must be upper-triangular with last row (0, 0, 1)")
    return np.ascontiguousarray(Km).reshape(-1), np.ascontiguousarray(lw).reshape(-1), len(lw)


class render_workspace:
    """Device scratch of dfh_render_raster / dfh_render_resolve for a (views, H, W, faces) size: the per-pixel keys and the list of
    large triangles.  mesh.render allocates one per call; a caller that renders the same size repeatedly may pass its own."""

    def __init__(self, n_views, H, W, n_faces, device=None):
        nbytes = _lib.load().dfh_render_workspace_bytes(int(n_views), int(H), int(W), int(n_faces))
        if nbytes == 0:
            raise ValueError("bad render size (views %d, %dx%d, %d faces)" % (n_views, H, W, n_faces))
        self.nbytes = nbytes
        self.buf = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device or "cuda")


def _rows3(a, what, dev):
    """(n,3) numpy array or tensor -> contiguous fp64 tensor on `dev`."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
    t = t.to(device=dev, dtype=torch.float64).contiguous()
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("%s must be (n,3), got shape %s" % (what, tuple(t.shape)))
    return t


def _render_args(verts, faces, K, lws, H, W, scale, center, half, znear, workspace):
    """What render and render_samples share: the arguments checked and on the device.  Returns (dev, V, F, mesh, views,
    workspace) with mesh = (verts pointer, n_verts, faces pointer, n_faces) and views = (n_views, K, lw, H, W, scale, center, half,
    znear, workspace pointer, workspace bytes) as the dfh_render_* calls take them."""
    Kf, lwf, nv = _view_table(K, lws)
    H, W = int(H), int(W)
    dev = torch.device("cuda", torch.cuda.current_device())
    V = _rows3(verts, "verts", dev)
    F = faces if isinstance(faces, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(faces)))
    F = F.to(device=dev, dtype=torch.int32).contiguous()
    if F.dim() != 2 or F.shape[1] != 3:
        raise ValueError("faces must be (n,3), got shape %s" % (tuple(F.shape),))
    ctr = np.broadcast_to(np.asarray(center, dtype=np.float64), (3,))
    if workspace is None:
        workspace = render_workspace(nv, H, W, F.shape[0], dev)
    views = (nv, _lib.darr(Kf, 9 * nv), _lib.darr(lwf, 12 * nv), H, W, float(scale), _lib.darr(ctr, 3), float(half), float(znear),
             workspace.buf.data_ptr(), workspace.buf.numel() * 8)
    return dev, V, F, (V.data_ptr(), V.shape[0], F.data_ptr(), F.shape[0]), views, workspace


def render(verts, faces, normals, K, lws, H, W, scale=1.0, center=0.0, half=0.0, znear=1e-3, workspace=None, stages=None):
    """Rasterise one triangle mesh into V views (csrc/dfh_render.hip, semantics in include/dfusion_hip.h): vertices (N,3) in
    voxel-index space, world = scale * (p - half) + center (K1's voxel -> world map), `lws` one 3x4 world->camera matrix or a list
    of V (one launch for all), K 3x3.  numpy arrays or CUDA tensors.  normals may be None.
    Returns (depth (V,H,W) fp32 = -z, 0 where no surface; normal (V,H,W,3) fp32 in the camera frame or None; face (V,H,W) int32,
    -1 where no surface) as CUDA tensors.  stages: optional callable(name) called after each of the two passes is enqueued
    (for timing tools)."""
    require_gpu()
    lib = _lib.load()
    dev, V, F, msh, views, workspace = _render_args(verts, faces, K, lws, H, W, scale, center, half, znear, workspace)
    nv, H, W = views[0], views[3], views[4]
    Nn = None if normals is None else _rows3(normals, "normals", dev)
    if Nn is not None and Nn.shape[0] != V.shape[0]:
        raise ValueError("normals and verts disagree in length")
    depth = torch.empty((nv, H, W), dtype=torch.float32, device=dev)
    face = torch.empty((nv, H, W), dtype=torch.int32, device=dev)
    normal = None if Nn is None else torch.empty((nv, H, W, 3), dtype=torch.float32, device=dev)
    _lib.check(lib.dfh_render_raster(*msh, *views, current_stream_ptr()), "dfh_render_raster")
    if stages is not None:
        stages("raster")
    _lib.check(lib.dfh_render_resolve(V.data_ptr(), 0 if Nn is None else Nn.data_ptr(), *msh[1:], *views, depth.data_ptr(), face.data_ptr(),
                                      0 if normal is None else normal.data_ptr(), current_stream_ptr()), "dfh_render_resolve")
    if stages is not None:
        stages("resolve")
    return depth, normal, face


def render_samples(verts, faces, canon_pos, canon_nrm, K, lws, H, W, scale=1.0, center=0.0, half=0.0, znear=1e-3, stride=1,
                   max_samples=None, workspace=None):
    """Visible-surface samples of one triangle mesh in V views (csrc/dfh_render.hip, semantics in include/dfusion_hip.h,
    dfh_render_samples_*): the mesh `verts` / `faces` is rasterised as by `render` (same arguments), and every `stride`-th pixel
    of every `stride`-th row that it covers yields one sample -- the per-vertex attributes `canon_pos` and `canon_nrm` ((N,3), the
    canonical mesh where `verts` is its warped copy; canon_nrm may be None) interpolated perspective-correctly at the pixel with
    the visible face's weights, the normal renormalised.  Samples come in view-major, then row, then column order.
    max_samples < the number of covered lattice pixels keeps extract_surface_samples' even subsample, never a prefix.
    Returns (pos (S,3) fp64, nrm (S,3) fp64 or None, pixel (S,) int64 = (view * H + y) * W + x) as CUDA tensors.  The raster pass,
    the count, one 8-byte read-back of the count, the emit pass."""
    require_gpu()
    lib = _lib.load()
    stride = int(stride)
    if stride < 1:
        raise ValueError("stride must be >= 1, got %d" % stride)
    if max_samples is not None and int(max_samples) < 0:
        raise ValueError("max_samples must be >= 0, got %d" % int(max_samples))
    dev, V, F, msh, views, workspace = _render_args(verts, faces, K, lws, H, W, scale, center, half, znear, workspace)
    nv, H, W = views[0], views[3], views[4]
    P = _rows3(canon_pos, "canon_pos", dev)
    Nn = None if canon_nrm is None else _rows3(canon_nrm, "canon_nrm", dev)
    if P.shape[0] != V.shape[0] or (Nn is not None and Nn.shape[0] != V.shape[0]):
        raise ValueError("canon_pos / canon_nrm and verts disagree in length")
    _lib.check(lib.dfh_render_raster(*msh, *views, current_stream_ptr()), "dfh_render_raster")
    sbytes = lib.dfh_render_samples_workspace_bytes(nv, H, W, stride)
    scan_buf = torch.empty((sbytes + 7) // 8, dtype=torch.int64, device=dev)
    scan = (scan_buf.data_ptr(), scan_buf.numel() * 8)
    total = HostScalar(torch.int64)                    # (the last scan launch stores the count straight into pinned host memory)
    _lib.check(lib.dfh_render_samples_count(nv, H, W, F.shape[0], stride, *views[-2:], *scan, total.ptr(), current_stream_ptr()),
               "dfh_render_samples_count")
    n = total.get()
    cap = n if max_samples is None else min(n, int(max_samples))
    pos = torch.empty((cap, 3), dtype=torch.float64, device=dev)
    nrm = None if Nn is None else torch.empty((cap, 3), dtype=torch.float64, device=dev)
    pixel = torch.empty((cap,), dtype=torch.int64, device=dev)
    _lib.check(lib.dfh_render_samples_emit(V.data_ptr(), P.data_ptr(), 0 if Nn is None else Nn.data_ptr(), *msh[1:], *views[:-2], stride,
                                           *views[-2:], *scan, pos.data_ptr(), 0 if nrm is None else nrm.data_ptr(), pixel.data_ptr(), cap,
                                           current_stream_ptr()), "dfh_render_samples_emit")
    return pos, nrm, pixel


RENDER_MAX_VIEWS = 16                                  # views per dfh_render_raster call


def render_vertex_ids(verts, faces, K, lws, H, W, znear_img, zfar_img, scale=1.0, center=0.0, half=0.0, znear=1e-3, workspace=None):
    """Vertex-id maps and 8-bit depth images of one triangle mesh in V views (csrc/dfh_render.hip, semantics in
    include/dfusion_hip.h, dfh_render_vertex_ids): the mesh is rasterised as by `render` (same arguments, K one 3x3 or one per
    view); every covered pixel whose depth lies in [znear_img, zfar_img] gets the vertex of the visible face with the largest
    perspective-correct barycentric coordinate and the grey level trunc(255 (zfar_img - z) / (zfar_img - znear_img)).
    Any number of views: the rasteriser takes 16 per call, the batches fill slices of one result.
    Returns (vid (V,H,W) int32, -1 where there is none; image (V,H,W) uint8, 0 there) as CUDA tensors."""
    require_gpu()
    lib = _lib.load()
    Kf, lwf, nv = _view_table(K, lws)
    Kf, lwf = Kf.reshape(nv, 3, 3), lwf.reshape(nv, 3, 4)
    H, W = int(H), int(W)
    dev = torch.device("cuda", torch.cuda.current_device())
    V = _rows3(verts, "verts", dev)
    vid = torch.empty((nv, H, W), dtype=torch.int32, device=dev)
    image = torch.empty((nv, H, W), dtype=torch.uint8, device=dev)
    for b0 in range(0, nv, RENDER_MAX_VIEWS):
        b1 = min(nv, b0 + RENDER_MAX_VIEWS)
        _, _, faces, msh, views, workspace = _render_args(V, faces, Kf[b0:b1], lwf[b0:b1], H, W, scale, center, half, znear, workspace)
        _lib.check(lib.dfh_render_raster(*msh, *views, current_stream_ptr()), "dfh_render_raster")
        _lib.check(lib.dfh_render_vertex_ids(*msh, *views, float(znear_img), float(zfar_img), vid[b0:b1].data_ptr(), image[b0:b1].data_ptr(),
                                             current_stream_ptr()), "dfh_render_vertex_ids")
    return vid, image


def depth_error(rendered, observed, gate):
    """Rendered against observed depth maps (reference storage convention: negative, 0 = none), per view: a list of dicts
    {n_valid: pixels valid in both, n_within: those with |difference| <= gate, mean, median: of |difference| over the valid
    pixels (torch's median: the lower middle value; nan when there are none)}.  (V,H,W) or (H,W) tensors / arrays."""
    r = rendered if isinstance(rendered, torch.Tensor) else torch.from_numpy(np.asarray(rendered))
    o = observed if isinstance(observed, torch.Tensor) else torch.from_numpy(np.asarray(observed))
    o = o.to(device=r.device, dtype=torch.float64)
    r = r.to(torch.float64)
    if r.shape != o.shape:
        raise ValueError("rendered %s and observed %s maps differ in shape" % (tuple(r.shape), tuple(o.shape)))
    if r.dim() == 2:
        r, o = r[None], o[None]
    out = []
    for v in range(r.shape[0]):
        valid = (r[v] != 0) & (o[v] != 0)
        d = (r[v] - o[v])[valid].abs()
        n = int(d.numel())
        out.append({"n_valid": n, "n_within": int((d <= gate).sum()) if n else 0,
                    "mean": float(d.mean()) if n else float("nan"), "median": float(d.median()) if n else float("nan")})
    return out


# ---------------------------------------------------------------------------------------------------------------- K22
# Mesh -> signed distance (csrc/dfh_mesh_sdf.hip; the result is defined in include/dfusion_hip.h).  The pseudonormal tables are
# built here, once per mesh, in numpy fp64 (the arccos stays on the host, so the device and tests/mesh_sdf_np.py read the same
# tables); everything per query point runs on the device.

def _mesh_arrays(verts, faces):
    v = verts.detach().cpu().numpy() if isinstance(verts, torch.Tensor) else np.asarray(verts)
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    if v.ndim != 2 or v.shape[1] != 3 or v.dtype not in (np.float32, np.float64):
        raise ValueError("verts must be (Nv, 3) float32 or float64")
    if f.ndim != 2 or f.shape[1] != 3 or not np.issubdtype(f.dtype, np.integer):
        raise ValueError("faces must be (F, 3) integer")
    if len(f) and (int(f.min()) < 0 or int(f.max()) >= len(v)):
        raise ValueError("faces hold a vertex index outside [0, %d)" % len(v))
    return np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int32)


def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def pseudonormals(verts, faces):
    """The angle-weighted pseudonormal tables of Baerentzen and Aanaes, fp64: (face_normals (F,3), edge_normals (F,3,3),
    vertex_normals (Nv,3), dropped (F,) bool).  dropped marks the faces whose ab x ac is the exact zero vector: they take part in
    nothing.  face: the unit normal.  edge, per (face, local edge AB / AC / BC): the sum of the unit normals of the kept faces
    sharing the undirected edge, in ascending face order (a boundary edge: the face's own).  vertex: the sum over the kept
    (face, corner) pairs at the vertex, in ascending (face, corner) order, of angle * unit normal, angle = arccos of the clipped
    cosine between the corner's two edges."""
    v, f = _mesh_arrays(verts, faces)
    A, B, C = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    ab, ac = B - A, C - A
    cr = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                   ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], axis=1)
    dropped = ~(cr != 0).any(axis=1)
    keep = np.flatnonzero(~dropped)
    fn = np.zeros((len(f), 3))
    en = np.zeros((len(f), 3, 3))
    vn = np.zeros((len(v), 3))
    if len(keep):
        with np.errstate(all="ignore"):
            fn[keep] = cr[keep] / np.sqrt(_dot3(cr[keep], cr[keep]))[:, None]
            fk = f[keep].astype(np.int64)
            # edges: items in (face, local edge) order, grouped by their undirected vertex pair
            pairs = np.stack([fk[:, [0, 1]], fk[:, [0, 2]], fk[:, [1, 2]]], axis=1).reshape(-1, 2)
            key = pairs.min(axis=1) * len(v) + pairs.max(axis=1)
            _, inv = np.unique(key, return_inverse=True)
            inv = inv.reshape(-1)
            acc = np.zeros((int(inv.max()) + 1, 3))
            np.add.at(acc, inv, np.repeat(fn[keep], 3, axis=0))
            en[keep] = acc[inv].reshape(-1, 3, 3)
            # vertices: items in (face, corner) order
            P = np.stack([A[keep], B[keep], C[keep]], axis=1)                  # (K, 3 corners, 3)
            u = np.stack([P[:, 1] - P[:, 0], P[:, 2] - P[:, 1], P[:, 0] - P[:, 2]], axis=1).reshape(-1, 3)
            w = np.stack([P[:, 2] - P[:, 0], P[:, 0] - P[:, 1], P[:, 1] - P[:, 2]], axis=1).reshape(-1, 3)
            cosang = _dot3(u, w) / (np.sqrt(_dot3(u, u)) * np.sqrt(_dot3(w, w)))
            ang = np.arccos(np.minimum(np.maximum(cosang, -1.0), 1.0))
            np.add.at(vn, fk.reshape(-1), ang[:, None] * np.repeat(fn[keep], 3, axis=0))
    return fn, en, vn, dropped


class MeshDistance:
    """A triangle mesh on the device, ready for exact distance queries: vertices widened to fp64, the pseudonormal tables, and
    the uniform cell table the query kernel walks.  orientation = +1: the faces wind outward (positive outside); cell: the table's
    cell edge (None: the library chooses); device: a CUDA device (None: the current one)."""

    def __init__(self, verts, faces, orientation=+1, cell=None, device=None):
        if orientation not in (1, -1):
            raise ValueError("orientation must be +1 or -1")
        v, f = _mesh_arrays(verts, faces)
        self.lib = lib = _lib.load()
        fn, en, vn, dropped = pseudonormals(v, f)
        keep = np.ascontiguousarray(~dropped, dtype=np.uint8)
        if cell is not None and not (np.isfinite(cell) and cell > 0):
            raise ValueError("cell must be finite and > 0")
        self.layout = lay = _lib.MeshSdfLayout()
        _lib.check(lib.dfh_mesh_sdf_plan(v.ctypes.data, len(v), f.ctypes.data, keep.ctypes.data, len(f), 0.0 if cell is None else float(cell),
                                         lay), "dfh_mesh_sdf_plan")
        require_gpu()
        self.device = dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.orientation = int(orientation)
        self.n_verts, self.n_faces, self.dropped = len(v), len(f), dropped
        with torch.cuda.device(dev):
            self._t = [torch.from_numpy(a).to(dev) for a in (v, f, keep, fn, en, vn)]
            self._table = torch.empty((lay.bytes + 7) // 8, dtype=torch.int64, device=dev)
            self._m = _lib.MeshSdf(*[t.data_ptr() for t in self._t], len(v), len(f), self._table.data_ptr(), self._table.numel() * 8, lay)
            _lib.check(lib.dfh_mesh_sdf_build(self._m, current_stream_ptr()), "dfh_mesh_sdf_build")

    @property
    def cell(self):
        return float(self.layout.cell)

    def query(self, points, band=float("inf")):
        """points (N, 3) -> (signed distance (N,) float64, closest point (N, 3) float32, face (N,) int32), device tensors.  A point
        farther than band: +band, NaN, -1."""
        p = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points, dtype=np.float64))
        if p.dim() != 2 or p.shape[1] != 3:
            raise ValueError("points must be (N, 3)")
        p = p.to(device=self.device, dtype=torch.float64).contiguous()
        n = p.shape[0]
        with torch.cuda.device(self.device):
            # a wave searches around the box of its 64 consecutive points: hand them over in Morton order of their table cells
            # (a point's result does not depend on its neighbours in the wave) and put the results back
            order = self._morton_order(p) if n > 64 else None
            q = p if order is None else p[order].contiguous()
            sd = torch.empty(n, dtype=torch.float64, device=self.device)
            cl = torch.empty((n, 3), dtype=torch.float32, device=self.device)
            fc = torch.empty(n, dtype=torch.int32, device=self.device)
            _lib.check(self.lib.dfh_mesh_sdf_points(self._m, q.data_ptr(), n, float(band), self.orientation, sd.data_ptr(), cl.data_ptr(),
                                                    fc.data_ptr(), current_stream_ptr()), "dfh_mesh_sdf_points")
            if order is not None:
                inv = torch.empty_like(order)
                inv[order] = torch.arange(n, device=self.device)
                sd, cl, fc = sd[inv], cl[inv], fc[inv]
        return sd, cl, fc

    def _morton_order(self, p):
        lay = self.layout
        lo = torch.tensor(list(lay.lo), dtype=torch.float64, device=self.device)
        c = torch.nan_to_num((p - lo) / lay.cell, nan=0.0).floor().clamp(-1.0, 1022.0).to(torch.int64) + 1          # 10 bits an axis
        for shift, mask in ((16, 0x30000FF), (8, 0x300F00F), (4, 0x30C30C3), (2, 0x9249249)):
            c = (c | (c << shift)) & mask
        return torch.argsort((c[:, 0] << 2) | (c[:, 1] << 1) | c[:, 2])

    def grid(self, origin, spacing, shape, band, dtype=np.float32, want_closest=False, want_face=False, out=None):
        """The signed distance on the grid origin + idx * spacing (scalars or 3-vectors), shape (X, Y, Z): a contiguous device
        volume of `dtype`; with a finite band the far vertices hold +-band, signed by the far fill (band >= max(spacing)).
        Returns the volume, then the closest points (X, Y, Z, 3) float32 and / or the faces (X, Y, Z) int32 if asked for."""
        shape = tuple(int(s) for s in shape)
        if len(shape) != 3:
            raise ValueError("shape must have three entries")
        dt = torch_dtype(dtype)
        if out is None:
            if min(shape) < 1:
                raise ValueError("shape entries must be at least 1")
            out = torch.empty(shape, dtype=dt, device=self.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and tuple(out.shape) == shape and out.dtype == dt):
            raise ValueError("out must be a contiguous device tensor of the grid's shape and dtype")
        g = _lib.MeshSdfGridParams()
        g.origin = (_lib._dbl * 3)(*np.broadcast_to(np.asarray(origin, dtype=np.float64), (3,)))
        g.spacing = (_lib._dbl * 3)(*np.broadcast_to(np.asarray(spacing, dtype=np.float64), (3,)))
        g.shape = _lib.iarr(shape)
        g.band, g.orientation, g.dtype, g.value = float(band), self.orientation, dtype_code(out), out.data_ptr()
        with torch.cuda.device(self.device):
            status = torch.empty(shape, dtype=torch.int8, device=self.device) if np.isfinite(band) else None
            cl = torch.empty(shape + (3,), dtype=torch.float32, device=self.device) if want_closest else None
            fc = torch.empty(shape, dtype=torch.int32, device=self.device) if want_face else None
            g.status = status.data_ptr() if status is not None else None
            g.closest = cl.data_ptr() if cl is not None else None
            g.face = fc.data_ptr() if fc is not None else None
            _lib.check(self.lib.dfh_mesh_sdf_grid(self._m, g, current_stream_ptr()), "dfh_mesh_sdf_grid")
        extras = tuple(t for t in (cl, fc) if t is not None)
        return (out,) + extras if extras else out



def surface_distance(points, verts, faces):
    """Unsigned distance (N,) float64 (device) from each point to the mesh's surface."""
    return MeshDistance(verts, faces).query(points)[0].abs()


def compare_meshes(verts_a, faces_a, verts_b, faces_b):
    """Vertex-to-surface distances both ways: accuracy (A's vertices to B's surface) and completeness (B's vertices to A's
    surface), each as mean, rms and max."""
    def stats(d):
        return {"mean": float(d.mean()), "rms": float(torch.sqrt((d * d).mean())), "max": float(d.max())}
    va, _ = _mesh_arrays(verts_a, faces_a)
    vb, _ = _mesh_arrays(verts_b, faces_b)
    return {"accuracy": stats(surface_distance(va, verts_b, faces_b)), "completeness": stats(surface_distance(vb, verts_a, faces_a))}


# ---------------------------------------------------------------------------------------------------------------- K23
# Connected components of a mesh (csrc/dfh_mesh_components.hip; every output is defined in include/dfusion_hip.h): labels, the
# per-component table and the compaction run on the device; which components to keep is decided from the table with torch.

class MeshComponents:
    """connected_components' result, CUDA tensors: n components; vert_comp (V,) / face_comp (F,) int32 component ids; per
    component root, n_verts, n_faces (int32), area (float64), bbox_min / bbox_max ((n, 3) float64).  vert_root (V,) int32 is
    the lowest vertex index of each vertex's component."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def _components_args(verts, faces):
    v = verts if isinstance(verts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(verts))
    f = faces if isinstance(faces, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(faces))
    if v.dim() != 2 or v.shape[1] != 3 or v.dtype not in (torch.float32, torch.float64):
        raise ValueError("verts must be (V, 3) float32 or float64")
    if f.dim() != 2 or f.shape[1] != 3 or f.dtype not in (torch.int32, torch.int64):
        raise ValueError("faces must be (F, 3) int32 or int64")
    if f.dtype == torch.int64 and f.numel() and (int(f.min()) < -(1 << 31) or int(f.max()) >= (1 << 31)):
        raise ValueError("faces hold an index that does not fit 32 bits")
    require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    return dev, v.to(dev).contiguous(), f.to(device=dev, dtype=torch.int32).contiguous()


def _components_workspace(lib, V, F, dev):
    nbytes = lib.dfh_mesh_components_workspace_bytes(V, F)
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)


def _ptr(t):
    return t.data_ptr() if t.numel() else None


def connected_components(verts, faces):
    """The connected components of a triangle mesh (two vertices are connected when a face names both): verts (V, 3) float32 /
    float64, faces (F, 3) integer, numpy arrays or tensors (moved to the current device) -> MeshComponents.  Component ids run in
    ascending order of the component's lowest vertex index; an unreferenced vertex is a component without faces.  A face index
    outside [0, V) raises ValueError.  The call waits for the label pass (it reads the component count back)."""
    lib = _lib.load()
    dev, v, f = _components_args(verts, faces)
    V, F = v.shape[0], f.shape[0]
    with torch.cuda.device(dev):
        ws = _components_workspace(lib, V, F, dev)
        root = torch.empty(V, dtype=torch.int32, device=dev)
        vert_comp = torch.empty(V, dtype=torch.int32, device=dev)
        face_comp = torch.empty(F, dtype=torch.int32, device=dev)
        n = ctypes.c_long(0)
        _lib.check(lib.dfh_mesh_components(_ptr(f), V, F, _ptr(root), _ptr(vert_comp), _ptr(face_comp), ctypes.byref(n), _ptr(ws),
                                           ws.numel() * 8, current_stream_ptr()), "dfh_mesh_components")
        C = int(n.value)
        croot = torch.empty(C, dtype=torch.int32, device=dev)
        nv = torch.empty(C, dtype=torch.int32, device=dev)
        nf = torch.empty(C, dtype=torch.int32, device=dev)
        bmin = torch.empty((C, 3), dtype=torch.float64, device=dev)
        bmax = torch.empty((C, 3), dtype=torch.float64, device=dev)
        area = torch.empty(C, dtype=torch.float64, device=dev)
        _lib.check(lib.dfh_mesh_component_table(_ptr(v), dtype_code(v), V, _ptr(f), F, _ptr(root), _ptr(vert_comp), _ptr(face_comp), C,
                                                _ptr(croot), _ptr(nv), _ptr(nf), _ptr(bmin), _ptr(bmax), _ptr(area), _ptr(ws), ws.numel() * 8,
                                                current_stream_ptr()), "dfh_mesh_component_table")
    return MeshComponents(n=C, vert_comp=vert_comp, face_comp=face_comp, vert_root=root, root=croot, n_verts=nv, n_faces=nf, area=area,
                          bbox_min=bmin, bbox_max=bmax, verts=v, faces=f)


def compact_components(comps, keep, drop_unreferenced=True):
    """The mesh of `comps` (a MeshComponents) cut down to the components with keep[c] != 0 ((n,) bool / uint8): (kept_vert_idx
    (V',) int32 = the surviving vertices' old indices, ascending; vert_map (V,) int32 = old -> new index, -1 for a dropped vertex;
    faces (F', 3) int32 = the surviving faces in their order, renumbered).  drop_unreferenced also removes the vertices of kept
    components that no surviving face names.  The call waits for the device (it reads the two counts back)."""
    lib = _lib.load()
    f, dev = comps.faces, comps.faces.device
    V, F, C = comps.vert_comp.shape[0], f.shape[0], comps.n
    k = keep if isinstance(keep, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(keep))
    k = (k.to(dev) != 0).to(torch.uint8).contiguous()
    if tuple(k.shape) != (C,):
        raise ValueError("keep must have one entry per component (%d), got shape %s" % (C, tuple(k.shape)))
    with torch.cuda.device(dev):
        ws = _components_workspace(lib, V, F, dev)
        kept = torch.empty(V, dtype=torch.int32, device=dev)
        vmap = torch.empty(V, dtype=torch.int32, device=dev)
        fout = torch.empty((F, 3), dtype=torch.int32, device=dev)
        counts = (ctypes.c_long * 2)(0, 0)
        _lib.check(lib.dfh_mesh_compact(_ptr(f), V, F, _ptr(comps.vert_comp), _ptr(comps.face_comp), _ptr(k), C, int(bool(drop_unreferenced)),
                                        _ptr(kept), _ptr(vmap), _ptr(fout), counts, _ptr(ws), ws.numel() * 8, current_stream_ptr()),
                   "dfh_mesh_compact")
    return kept[:counts[0]], vmap, fout[:counts[1]]


def keep_mask(comps, min_faces=0, min_area=0.0, keep_largest=None):
    """Which components filter_components keeps, (n,) bool on the device: n_faces >= min_faces, area not below min_area and, with
    keep_largest = k, among the k components with the most faces (ties go to the lower id)."""
    keep = (comps.n_faces >= int(min_faces)) & ~(comps.area < float(min_area))        # (a NaN area is not below the bound)
    if keep_largest is not None:
        k = int(keep_largest)
        if k < 0:
            raise ValueError("keep_largest must be >= 0, got %d" % k)
        order = torch.sort(comps.n_faces, descending=True, stable=True).indices[:k]
        top = torch.zeros_like(keep)
        top[order] = True
        keep = keep & top
    return keep


def filter_components(verts, faces, *attrs, min_faces=0, min_area=0.0, keep_largest=None, drop_unreferenced=True):
    """Drop the fragments of a mesh: keeps the components keep_mask() selects and returns (verts, faces, *attrs, kept_vert_idx)
    as CUDA tensors -- vertex and face order preserved, faces renumbered, every per-vertex attribute in `attrs` ((V, ...) arrays or
    tensors: normals, values, colours, canonical positions) gathered with kept_vert_idx (int64 here, ready to index with).
    drop_unreferenced also removes the vertices no surviving face names."""
    comps = connected_components(verts, faces)
    V = comps.vert_comp.shape[0]
    kept, _, f2 = compact_components(comps, keep_mask(comps, min_faces, min_area, keep_largest), drop_unreferenced)
    idx = kept.long()
    out = []
    for a in attrs:
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        if t.shape[0] != V:
            raise ValueError("an attribute has %d rows for %d vertices" % (t.shape[0], V))
        out.append(t.to(comps.verts.device)[idx])
    return (comps.verts[idx], f2, *out, idx)


# ---------------------------------------------------------------------------------------------------------------- K24
# Simplification by vertex clustering with quadrics (csrc/dfh_mesh_simplify.hip; every output is defined in include/dfusion_hip.h).
# The two groupings are stable torch.sorts (the int64 cell keys; the 3F corner entries by the vertex they name), plumbing as
# graph.py's; keys, cluster ids, quadrics, the solve, the face tests and the compaction run in the kernels.

_SIMPLIFY_MODES = {"quadric": 0, "mean": 1}


def _simplify_attr(a, V):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError("a per-vertex attribute must be float32 or float64, got %s" % t.dtype)
    if t.dim() < 1 or t.shape[0] != V:
        raise ValueError("an attribute has %d rows for %d vertices" % (t.shape[0] if t.dim() else 0, V))
    return t


def simplify(verts, faces, *attrs, cell, origin=None, mode="quadric", reg=1e-3, drop_unreferenced=True):
    """A coarser mesh by vertex clustering: the vertices that share a cell of the grid (origin, cell) become one vertex -- the
    minimiser of the cluster's summed face-plane quadric, regularised by reg towards the cluster's mean and kept inside the cell
    (mode "quadric": sharp features survive), or the mean itself (mode "mean") -- faces are remapped, those that collapse or
    repeat an earlier face's vertex triple are dropped.  verts (V, 3) float32 / float64, faces (F, 3) int32 / int64, numpy arrays
    or tensors; attrs: per-vertex (V, ...) float32 / float64 arrays, averaged per cluster in fp64; origin: 3 numbers, default the
    per-axis minimum of verts.  -> (verts', faces', *attrs', info) as CUDA tensors; info: vert_map (V,) int64 old vertex -> new
    vertex (-1 where dropped), face_idx (F',) int64 old face indices, n_clusters (before drop_unreferenced removes the clusters no
    surviving face names), n_fallback (the clusters whose quadric solve was refused and that took the mean).
    The result is a function of the inputs alone, bit for bit.  It is not guaranteed manifold or consistently oriented where
    sheets thinner than a cell collapse: two sides of a thin sheet become the same triangle twice, with opposite orientation, and
    the one with the lower index survives.  A coordinate that is not finite, a vertex further than 2^21 cells from the origin (or
    below it) and a face index outside [0, V) raise ValueError.  The call waits for the device three times (it reads counts)."""
    if mode not in _SIMPLIFY_MODES:
        raise ValueError("mode must be 'quadric' or 'mean', got %r" % (mode,))
    cell, reg = float(cell), float(reg)
    if not (np.isfinite(cell) and cell > 0.0):
        raise ValueError("cell must be a finite number above 0, got %r" % cell)
    if not (np.isfinite(reg) and reg >= 0.0):
        raise ValueError("reg must be a finite number that is not negative, got %r" % reg)
    V = verts.shape[0] if hasattr(verts, "shape") and len(verts.shape) else 0
    attrs = [_simplify_attr(a, V) for a in attrs]
    lib = _lib.load()
    dev, v, f = _components_args(verts, faces)
    V, F = v.shape[0], f.shape[0]
    attrs = [a.to(dev).contiguous() for a in attrs]
    if origin is None:
        o = v.double().amin(dim=0).cpu().numpy() if V else np.zeros(3)
    else:
        o = np.asarray(origin, dtype=np.float64).reshape(-1)
        if o.shape != (3,):
            raise ValueError("origin must be 3 numbers")
    org = (ctypes.c_double * 3)(*[float(x) for x in o])
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = current_stream_ptr()
        nbytes = lib.dfh_mesh_simplify_workspace_bytes(V, F)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        wsb = ws.numel() * 8
        keys = torch.empty(V, dtype=torch.int64, device=dev)
        _lib.check(lib.dfh_mesh_simplify_keys(_ptr(v), dtype_code(v), V, _ptr(f), F, cell, org, _ptr(keys), _ptr(ws), wsb, stream),
                   "dfh_mesh_simplify_keys")
        skeys, order = torch.sort(keys, stable=True)
        scv, corder = torch.sort(f.reshape(-1), stable=True)
        vclus, cstart, ccount, cbeg, cend = i32(V), i32(V), i32(V), i32(V), i32(V)
        n = ctypes.c_long(0)
        _lib.check(lib.dfh_mesh_simplify_group(_ptr(skeys), _ptr(order), V, _ptr(scv), F, _ptr(vclus), _ptr(cstart), _ptr(ccount), _ptr(cbeg),
                                               _ptr(cend), ctypes.byref(n), _ptr(ws), wsb, stream), "dfh_mesh_simplify_group")
        C = int(n.value)
        cverts = torch.empty((C, 3), dtype=v.dtype, device=dev)
        nfb = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(lib.dfh_mesh_simplify_clusters(_ptr(v), dtype_code(v), V, _ptr(f), F, cell, org, _SIMPLIFY_MODES[mode], reg, _ptr(keys),
                                                  _ptr(order), _ptr(corder), _ptr(cbeg), _ptr(cend), _ptr(cstart), _ptr(ccount), C, _ptr(cverts),
                                                  _ptr(nfb), _ptr(ws), wsb, stream), "dfh_mesh_simplify_clusters")
        cattrs = []
        for a in attrs:
            out = torch.empty((C,) + tuple(a.shape[1:]), dtype=a.dtype, device=dev)
            K = a.numel() // V if V else 0
            _lib.check(lib.dfh_mesh_simplify_attr(_ptr(a), dtype_code(a), V, K, _ptr(order), _ptr(cstart), _ptr(ccount), C, _ptr(out), stream),
                       "dfh_mesh_simplify_attr")
            cattrs.append(out)
        fout, fidx, cmap, kept, vmap = i32(F, 3), i32(F), i32(C), i32(C), i32(V)
        counts = (ctypes.c_long * 2)(0, 0)
        _lib.check(lib.dfh_mesh_simplify_faces(_ptr(f), V, F, _ptr(vclus), C, int(bool(drop_unreferenced)), _ptr(fout), _ptr(fidx), _ptr(cmap),
                                               _ptr(kept), _ptr(vmap), counts, _ptr(ws), wsb, stream), "dfh_mesh_simplify_faces")
        idx = kept[:counts[0]].long()
        info = {"vert_map": vmap.long(), "face_idx": fidx[:counts[1]].long(), "n_clusters": C, "n_fallback": int(nfb.item())}
    return (cverts[idx], fout[:counts[1]], *[a[idx] for a in cattrs], info)


def simplify_with_normals(verts, faces, normals, cell, **kw):
    """simplify() for a mesh that carries vertex normals: the normals are averaged per cluster as an attribute and brought back to
    unit length (a normal that averages to zero stays zero) -> (verts', faces', normals', info).  What the simplify_cell hooks of
    Fusion / FusionDM.write_canonical_mesh and SlabFrame.colored_mesh run."""
    v, f, n, info = simplify(verts, faces, normals, cell=cell, **kw)
    length = torch.linalg.vector_norm(n, dim=1, keepdim=True)
    return v, f, torch.where(length > 0, n / length, torch.zeros_like(n)), info


# ---------------------------------------------------------------------------------------------------------------- K25
# Smoothing by Taubin's lambda|mu filter over a fixed Laplacian, and area-weighted vertex normals (csrc/dfh_mesh_smooth.hip;
# every output is defined in include/dfusion_hip.h).  The grouping is K24's stable torch.sort of the 3F corner entries by the
# vertex they name, plumbing; the neighbour lists, the boundary flags, the weights and every pass run in the kernels.

_SMOOTH_WEIGHTS = {"uniform": 0, "cotangent": 1}
_SMOOTH_BOUNDARY = {"fixed": 0, "free": 1}
_SMOOTH_LAYOUTS = {"rows": 0, "planes": 1}


def taubin_mu(lam, pass_band):
    """The negative factor of Taubin's filter for a positive factor lam and a pass-band frequency: 1 / (pass_band - 1 / lam), in
    Python floats (fp64)."""
    lam, pass_band = float(lam), float(pass_band)
    if not (np.isfinite(lam) and lam != 0.0 and np.isfinite(pass_band)) or pass_band - 1.0 / lam == 0.0:
        raise ValueError("mu = 1 / (pass_band - 1 / lam) needs a finite lam that is not 0 and pass_band != 1 / lam, got lam %r, pass_band %r"
                         % (lam, pass_band))
    return 1.0 / (pass_band - 1.0 / lam)


class MeshLaplacian:
    """A triangle mesh on the device with its prepared adjacency: per vertex the list of its faces' other two corners, the
    boundary flags and (weights "cotangent") the cotangent weights of the positions given here, clamped at 0.  verts (V, 3)
    float32 / float64, faces (F, 3) int32 / int64, numpy arrays or tensors (moved to the current device).  weights "uniform": a
    neighbour counts once per face sharing the edge (the umbrella operator on a closed manifold).  boundary "fixed": a flagged
    vertex never moves; "free": it moves like any other (and an open rim shrinks).  .boundary: (V,) bool, True where the vertex
    lies on an open, non-manifold or repeated edge.  The operator is fixed: smooth() never recomputes the weights.  A coordinate
    that is not finite and a face index outside [0, V) raise ValueError.  The constructor waits for the device once."""

    layout = "rows"                      # how the fp64 values lie between passes ("rows" / "planes": the same bits; profiles/r29_smooth.txt)

    def __init__(self, verts, faces, weights="uniform", boundary="fixed"):
        if weights not in _SMOOTH_WEIGHTS:
            raise ValueError("weights must be 'uniform' or 'cotangent', got %r" % (weights,))
        if boundary not in _SMOOTH_BOUNDARY:
            raise ValueError("boundary must be 'fixed' or 'free', got %r" % (boundary,))
        self.lib = lib = _lib.load()
        self.device, self.verts, self.faces = dev, v, f = _components_args(verts, faces)
        self.weights, self.boundary_mode = weights, boundary
        self.n_verts, self.n_faces = V, F = v.shape[0], f.shape[0]
        with torch.cuda.device(dev):
            scv, corder = torch.sort(f.reshape(-1), stable=True)
            nbytes = lib.dfh_mesh_smooth_workspace_bytes(V, F)
            if F and not nbytes:
                raise ValueError("a mesh of %d vertices and %d faces is too large (3F must fit an int)" % (V, F))
            self._ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
            flags = torch.zeros(V, dtype=torch.uint8, device=dev)
            _lib.check(lib.dfh_mesh_smooth_prepare(_ptr(v), dtype_code(v), V, _ptr(f), F, _ptr(scv), _ptr(corder), _SMOOTH_WEIGHTS[weights],
                                                   _ptr(flags), _ptr(self._ws), self._ws.numel() * 8, current_stream_ptr()),
                       "dfh_mesh_smooth_prepare")
        self.boundary = flags.bool()

    def _rows(self, x, what):
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        if t.dtype not in (torch.float32, torch.float64):
            raise ValueError("%s must be float32 or float64, got %s" % (what, t.dtype))
        if t.dim() not in (1, 2) or t.shape[0] != self.n_verts:
            raise ValueError("%s must have one row per vertex (%d), got shape %s" % (what, self.n_verts, tuple(t.shape)))
        return t.to(self.device).contiguous()

    def smooth(self, x=None, iters=10, lam=0.5, mu=None, pass_band=0.1):
        """iters times (a pass with factor lam, then one with factor mu) over x: None = the vertices given to the constructor, or
        a per-vertex attribute (V,) / (V, K), K <= 4, float32 / float64, filtered by the same operator.  mu None: Taubin's
        1 / (pass_band - 1 / lam), which keeps the volume; mu = 0: plain Laplacian smoothing, which shrinks.  -> a CUDA tensor of
        x's shape and dtype (fp64 inside, rounded once).  The call only enqueues."""
        iters, lam = int(iters), float(lam)
        mu = taubin_mu(lam, pass_band) if mu is None else float(mu)
        if iters < 0:
            raise ValueError("iters must not be negative, got %d" % iters)
        if not (np.isfinite(lam) and np.isfinite(mu)):
            raise ValueError("lam and mu must be finite, got %r and %r" % (lam, mu))
        t = self.verts if x is None else self._rows(x, "x")
        K = 1 if t.dim() == 1 else t.shape[1]
        if not 1 <= K <= 4:
            raise ValueError("x must have 1 to 4 columns, got %d" % K)
        with torch.cuda.device(self.device):
            out = torch.empty_like(t)
            _lib.check(self.lib.dfh_mesh_smooth_run(_ptr(t), dtype_code(t), self.n_verts, self.n_faces, K, _SMOOTH_WEIGHTS[self.weights],
                                                    _SMOOTH_BOUNDARY[self.boundary_mode], _SMOOTH_LAYOUTS[self.layout], iters, lam, mu, _ptr(out),
                                                    _ptr(self._ws), self._ws.numel() * 8, current_stream_ptr()), "dfh_mesh_smooth_run")
        return out

    def vertex_normals(self, verts=None, sign=1.0):
        """Area-weighted unit vertex normals of `verts` (None: the constructor's; or moved ones, e.g. smooth()'s) over this mesh's
        faces: the sum of the faces' (p_a - p_v) x (p_b - p_v) at each vertex, times sign, normalised; zero where that sum is
        zero.  sign = +1: the winding's right-hand normal.  -> (V, 3) CUDA tensor of the verts' dtype.  The call only enqueues."""
        sign = float(sign)
        if not np.isfinite(sign):
            raise ValueError("sign must be finite, got %r" % sign)
        t = self.verts if verts is None else self._rows(verts, "verts")
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("verts must be (V, 3)")
        with torch.cuda.device(self.device):
            out = torch.empty_like(t)
            _lib.check(self.lib.dfh_mesh_vertex_normals(_ptr(t), dtype_code(t), self.n_verts, self.n_faces, sign, _ptr(out), _ptr(self._ws),
                                                        self._ws.numel() * 8, current_stream_ptr()), "dfh_mesh_vertex_normals")
        return out


def smooth(verts, faces, iters=10, weights="uniform", boundary="fixed", **kw):
    """The vertices of a mesh after `iters` Taubin iterations (MeshLaplacian(verts, faces, weights, boundary).smooth(None, iters,
    **kw)): voxel-scale ripple goes, the volume stays.  -> (V, 3) CUDA tensor of the verts' dtype; the faces are unchanged."""
    return MeshLaplacian(verts, faces, weights, boundary).smooth(None, iters, **kw)


def vertex_normals(verts, faces, sign=1.0):
    """Area-weighted unit vertex normals recomputed from the faces (MeshLaplacian.vertex_normals) -> (V, 3) CUDA tensor."""
    return MeshLaplacian(verts, faces).vertex_normals(None, sign)


def smooth_with_normals(verts, faces, iters, **kw):
    """smooth() for a mesh that carries vertex normals: -> (verts', normals'), the normals recomputed from the moved vertices
    with sign = -1 (this project's marching-cubes normals point against the winding's right-hand normal).  What the smooth_iters
    hooks of Fusion / FusionDM.write_canonical_mesh and SlabFrame.colored_mesh run."""
    lap = MeshLaplacian(verts, faces, kw.pop("weights", "uniform"), kw.pop("boundary", "fixed"))
    moved = lap.smooth(None, iters, **kw)
    return moved, lap.vertex_normals(moved, -1.0)
