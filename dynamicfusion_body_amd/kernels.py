"""Tensor-level entry points: device tensors in, updated in place, asynchronous on the
current HIP stream.  Each function is one call through the C ABI (include/dfusion_hip.h);
the reference-shaped classes in fusion_dm.py / fusion.py are built on these."""
import ctypes
import numpy as np
import torch

from . import _lib
from .device import current_stream_ptr, dtype_code, require_gpu


def _check_volume_pair(T, Wt, res, x_range):
    if not (isinstance(T, torch.Tensor) and isinstance(Wt, torch.Tensor)):
        raise ValueError("volumes must be torch tensors on the GPU")
    if not (T.is_cuda and Wt.is_cuda):
        raise ValueError("volumes must live on the GPU")
    if T.dtype != Wt.dtype:
        raise ValueError("tsdf and weight volumes must share a dtype")
    if not (T.is_contiguous() and Wt.is_contiguous()):
        raise ValueError("volumes must be contiguous [x][y][z]")
    x0, x1 = x_range
    want = (x1 - x0, res[1], res[2])
    if tuple(T.shape) != want or tuple(Wt.shape) != want:
        raise ValueError("volume shape %s / %s does not match slab %s of grid %s"
                         % (tuple(T.shape), tuple(Wt.shape), want, tuple(res)))


def _volume(T, Wt, res, x_range, tsdf_res=None):
    """The defaults every K1-K3 entry point applies (the whole grid, all its planes, tsdf_res = res[0]), the volume pair's checks
    and the dfh_volume of the call: (dfh_volume, tsdf_res)."""
    if res is None:
        res = tuple(T.shape)
    _check_volume_pair(T, Wt, res, (0, res[0]) if x_range is None else x_range)
    vol = _lib.Volume(T.data_ptr(), Wt.data_ptr(), dtype_code(T), _lib.slab(res, x_range))
    return vol, int(res[0] if tsdf_res is None else tsdf_res)


def _check_depth(d):
    if not (isinstance(d, torch.Tensor) and d.is_cuda and d.dim() == 2 and d.is_contiguous()):
        raise ValueError("depth must be a contiguous 2-D CUDA tensor")


def _view_batches(depths, lws, K, Kinv, scale, center, on_gpu=False):
    """The depth maps of one call: checks that they are 2-D tensors of one shape and dtype (on_gpu: _check_depth on each instead
    of the first half, for callers that already hold a device) and returns batches(tsdf_res), a generator of (i, dfh_depth_views)
    over the maps [i, i + 16) -- the most one library call takes."""
    for d in depths:
        if on_gpu:
            _check_depth(d)
        elif not (isinstance(d, torch.Tensor) and d.dim() == 2):
            raise ValueError("depth must be a contiguous 2-D CUDA tensor")
        if d.shape != depths[0].shape or d.dtype != depths[0].dtype:
            raise ValueError("all depth maps of one call must have the same shape and dtype")

    def batches(tsdf_res):
        H, W = depths[0].shape
        for i in range(0, len(depths), 16):
            dd = depths[i:i + 16]
            n = len(dd)
            ptrs = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dd])
            lw = _lib.darr(np.concatenate([np.asarray(l, dtype=np.float64).reshape(12) for l in lws[i:i + 16]]), 12 * n)
            yield i, _lib.DepthViews(n, ptrs, dtype_code(dd[0]), int(H), int(W), _lib.darr(K, 9), _lib.darr(Kinv, 9), lw, float(scale),
                                     _lib.darr(np.asarray(center, dtype=np.float64), 3), tsdf_res)
    return batches


def _integrate(vol, views, tdist, wmax, fresh, workspace):
    """One dfh_integrate_depth call: the maps of `views` (one batch of _view_batches) into `vol`."""
    ws_ptr, ws_bytes = (workspace.data_ptr(), workspace.numel() * workspace.element_size()) if isinstance(workspace, torch.Tensor) else (0, 0)
    rc = _lib.load().dfh_integrate_depth(vol, views, float(tdist), float(wmax), None if fresh is None else ctypes.c_double(float(fresh)),
                                         ws_ptr, ws_bytes, current_stream_ptr())
    _lib.check(rc, "dfh_integrate_depth")


_ws_cache = {}


def integrate_workspace(n_views, H, W, res, x_range=None, device=None):
    """Scratch tensor for integrate_depth / integrate_depth_views on planes `x_range` of a `res` grid (the views'
    parameters, depth pyramids and per-brick view masks); cached per (device, stream, n_views, H, W, grid, slab size):
    launches on one stream are ordered, so consecutive calls may share it."""
    lib = _lib.load()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if x_range is None:
        x_range = (0, res[0])
    nx = int(x_range[1]) - int(x_range[0])
    key = (dev.index, current_stream_ptr(), int(n_views), int(H), int(W), int(res[1]), int(res[2]), nx)
    ws = _ws_cache.get(key)
    if ws is None:
        nbytes = lib.dfh_integrate_workspace_bytes(int(n_views), int(H), int(W), _lib.slab(res, (0, nx)))
        ws = torch.empty((nbytes + 15) // 16 * 2, dtype=torch.int64, device=dev)
        if len(_ws_cache) > 64:
            _ws_cache.clear()
        _ws_cache[key] = ws
    return ws


K1_PATHS = {0: "exact", 1: "rows", 2: "columns", 3: "columns_culled"}       # include/dfusion_hip.h: DFH_K1_PATH_*
BRICK = (4, 2, 32)                                                            # voxels of a brick of the column sweep (csrc/dfh_integrate.hip)


def integrate_path(T, depth, res=None, x_range=None, workspace=True):
    """The byte class of the sweep integrate_depth takes for this slab and depth map (dfh_integrate_depth_path; no launch):
    "rows" = T and w loaded and stored for the updated packs only (the row sweep, and the gather-first column walk that 256^3
    slabs take), "columns" = T and w of every pack loaded, "columns_culled" = of every pack of the bricks the culling passes
    keep, "exact" = the fp64 chain."""
    lib = _lib.load()
    if res is None:
        res = tuple(T.shape)
    H, W = depth.shape
    code = lib.dfh_integrate_depth_path(dtype_code(T), _lib.slab(res, x_range), int(H), int(W), 1 if workspace else 0)
    if code < 0:
        _lib.check(code, "dfh_integrate_depth_path")
    return K1_PATHS[code]


def brick_masks(workspace, res, x_range=None):
    """The per-brick 16-bit view masks the last culled sweep through `workspace` left behind (bit v = view v may update a voxel
    of the brick), as a (bricks_x, bricks_y, bricks_z) int16 view: the LAST region of the workspace (include/dfusion_hip.h:
    dfh_integrate_workspace_bytes).  Measurement code counts surviving bricks with it."""
    if x_range is None:
        x_range = (0, res[0])
    nb = (-(-(int(x_range[1]) - int(x_range[0])) // BRICK[0]), -(-int(res[1]) // BRICK[1]), -(-int(res[2]) // BRICK[2]))
    n = nb[0] * nb[1] * nb[2]
    raw = workspace.view(torch.int16)
    tail = (2 * n + 15) // 16 * 8                       # the mask region is padded to whole 16-byte units
    return raw[raw.numel() - tail:raw.numel() - tail + n].view(nb)


def integrate_workspace_params_doubles(workspace, n_views):
    """The views' parameter records the last multi-view sweep through `workspace` uploaded, as an (n_views, record) float64 view:
    the FIRST region of the workspace (dfh_integrate_multi_workspace_bytes(n) bytes, rounded to 16; a record starts with K, K^-1 and
    lw).  Single-view sweeps never write it.  For tests that must know which path a call took."""
    rec = _lib.load().dfh_integrate_multi_workspace_bytes(2) // 16           # doubles per record (two records need no padding)
    return workspace.view(torch.float64)[:rec * int(n_views)].view(int(n_views), rec)


def integrate_depth(T, Wt, depth, K, Kinv, lw, scale, center, tdist, wmax=100.0, tsdf_res=None,
                    res=None, x_range=None, workspace=None):
    """K1 = FusionDM.fuseDepths (reference core/fusion_dm.py:180-217) on device tensors.

    T, Wt : (x1-x0, Y, Z) float32/float64 CUDA tensors holding planes [x0,x1) of a `res`
            grid (default: the whole grid).  depth: (H, W) float32/float64 CUDA tensor of
            negative depths.  Runs asynchronously on the current stream.  workspace: scratch from
            integrate_workspace(1, H, W) (default: a cached one); False = sweep without brick culling."""
    require_gpu()
    vol, tsdf_res = _volume(T, Wt, res, x_range, tsdf_res)
    if vol.slab.x1 == vol.slab.x0:
        return T, Wt
    batches = _view_batches([depth], [lw], K, Kinv, scale, center, on_gpu=True)
    if workspace is None and T.dtype == torch.float32:
        workspace = integrate_workspace(1, *depth.shape, vol.slab.res, (vol.slab.x0, vol.slab.x1), T.device)
    _integrate(vol, next(batches(tsdf_res))[1], tdist, wmax, None, workspace)
    return T, Wt


def integrate_depth_ocl(T, Wt, depth, proj, kinv_row2, tdist, wmax=100.0, res=None, x_range=None):
    """A2: the arithmetic of the reference's OpenCL kernel (core/fusion_dm.py:630-674; dfh_integrate_depth_ocl) on float32
    device volumes, in place.  proj: float32 3x4 index -> pixel map (K lw IND, :695); kinv_row2: third row of K^-1 (float32)."""
    require_gpu()
    lib = _lib.load()
    vol, _ = _volume(T, Wt, res, x_range)
    if T.dtype != torch.float32:
        raise ValueError("the OpenCL arithmetic is float32: volumes must be float32")
    if not (isinstance(depth, torch.Tensor) and depth.is_cuda and depth.dim() == 2 and depth.is_contiguous() and depth.dtype == torch.float32):
        raise ValueError("depth must be a contiguous 2-D float32 CUDA tensor")
    if vol.slab.x1 == vol.slab.x0:
        return T, Wt
    pr = (ctypes.c_float * 12)(*np.asarray(proj, dtype=np.float32).reshape(12).tolist())
    kr = (ctypes.c_float * 3)(*np.asarray(kinv_row2, dtype=np.float32).reshape(3).tolist())
    H, W = depth.shape
    _lib.check(lib.dfh_integrate_depth_ocl(vol, depth.data_ptr(), int(H), int(W), pr, kr, ctypes.c_float(float(tdist)),
                                           ctypes.c_float(float(wmax)), current_stream_ptr()), "dfh_integrate_depth_ocl")
    return T, Wt


def integrate_depth_views(T, Wt, depths, K, Kinv, lws, scale, center, tdist, wmax=100.0, tsdf_res=None, res=None,
                          x_range=None, workspace=None, fresh=None):
    """Several views in one sweep of the volume (dfh_integrate_depth with n_views > 1): same result, bit for bit, as
    integrate_depth called once per view in this order (what the reference's loops over fuseDepths do,
    core/fusion_dm.py:152-154,166-170), with T and w read and written once.  depths: list of (H, W) CUDA tensors of one
    shape and dtype; lws: list of 3x4 extrinsics.  More than 16 views are taken 16 at a time.
    fresh=value: T and Wt are first set to (value, 0) -- a live volume from scratch, core/fusion_dm.py:152-153 -- as part of the
    same sweep (dfh_integrate_depth's fresh_value): what T.fill_(value); Wt.zero_() in front of this call give, bit for bit."""
    require_gpu()
    lib = _lib.load()
    depths, lws = list(depths), list(lws)
    if len(depths) != len(lws):
        raise ValueError('length of camera matrix array must equal that of depth maps')        # core/fusion_dm.py:96-97
    vol, tsdf_res = _volume(T, Wt, res, x_range, tsdf_res)
    if vol.slab.x1 == vol.slab.x0:
        return T, Wt
    if not depths:
        if fresh is not None:
            T.fill_(float(fresh))
            Wt.zero_()
        return T, Wt
    batches = _view_batches(depths, lws, K, Kinv, scale, center, on_gpu=True)
    H, W = depths[0].shape
    slab = vol.slab
    for i, views in batches(tsdf_res):
        nbytes = lib.dfh_integrate_workspace_bytes(views.n_views, int(H), int(W), slab)
        ws = workspace if (workspace is not None and workspace.numel() * workspace.element_size() >= nbytes) else \
            integrate_workspace(views.n_views, H, W, slab.res, (slab.x0, slab.x1), T.device)
        _integrate(vol, views, tdist, wmax, fresh if i == 0 else None, ws)
    return T, Wt


def _check_live(live):
    if not (isinstance(live, torch.Tensor) and live.is_cuda and live.dim() == 3 and live.is_contiguous()):
        raise ValueError("live TSDF must be a contiguous 3-D CUDA tensor")
    return _lib.Live(live.data_ptr(), dtype_code(live), _lib.iarr(live.shape))


def fuse_volume_rigid(T, Wt, live, lw_dq, tdist, wmax=100.0, res=None, x_range=None):
    """K2 = FusionDM.updateTSDF (reference core/fusion_dm.py:300-316) on device tensors.
    T, Wt: planes [x0,x1) of the canonical grid `res`; live: the whole live volume."""
    require_gpu()
    lib = _lib.load()
    vol, _ = _volume(T, Wt, res, x_range)
    live = _check_live(live)
    if vol.slab.x1 == vol.slab.x0:
        return T, Wt
    rc = lib.dfh_fuse_volume_rigid(vol, live, _lib.darr(lw_dq, 8), float(tdist), float(wmax), current_stream_ptr())
    _lib.check(rc, "dfh_fuse_volume_rigid")
    return T, Wt


def dqb_workspace(res, x_range=None, device=None, knn=None, n_nodes=None, level=2):
    """Scratch tensor for fuse_volume_dqb: the per-brick candidate node lists and, when `knn` and `n_nodes` are
    given, per voxel the knn node indices (level 1: 2*knn bytes) and blend weights (level 2: + 8*(knn+1) bytes);
    calls with rebuild_candidates=False then skip the node search / the weight computation."""
    require_gpu()
    lib = _lib.load()
    if knn is not None and n_nodes is not None:
        nbytes = lib.dfh_dqb_workspace_bytes_cached(_lib.slab(res, x_range), int(knn), int(n_nodes), int(level))
    else:
        nbytes = lib.dfh_dqb_workspace_bytes(_lib.slab(res, x_range))
    return torch.empty(max(1, (nbytes + 3) // 4), dtype=torch.int32, device=device or "cuda")


def dqb_skip_tables(workspace, res, live_res, n_nodes, x_range=None, knn=4):
    """Views of the constant-live skip's per-call tables inside a level-2 dqb_workspace (dfh_dqb_skip_layout), as left by the last
    steady-state fuse_volume_dqb call through it: {"U": live-cell mask words, "S": uint8 per brick (1 = its voxels took the constant-live stream), "reach": uint8 per
    brick, "bound": float32 per brick (voxels; -1 = not computed: the live volume ruled the skip out; option k3_skip = 2 computes all), "used": int16 (bricks, 16) node ids, "n_listed": 16-voxel rows left to the warp kernel, "n_runs": all such rows, "ok": sizes admit the skip}.  For tests and
    measurement code."""
    lib = _lib.load()
    if x_range is None:
        x_range = (0, res[0])
    out = (ctypes.c_size_t * 13)()
    _lib.check(lib.dfh_dqb_skip_layout(_lib.slab(res, x_range), _lib.iarr(live_res), int(knn), int(n_nodes), out), "dfh_dqb_skip_layout")
    raw = workspace.view(torch.uint8)
    nx = int(x_range[1]) - int(x_range[0])
    nb = (-(-nx // 4)) * (-(-int(res[1]) // 4)) * (-(-int(res[2]) // 16))
    CX, CY, WZ, SCX, SCY = (int(out[i]) for i in (6, 7, 8, 9, 10))
    n_runs = nx * int(res[1]) * (int(res[2]) // 16)                      # 16-voxel rows

    def region(i, nbytes, dtype):
        return raw[int(out[i]):int(out[i]) + nbytes].view(dtype)
    tabs = {"ok": bool(out[11]), "U": region(0, CX * CY * WZ * 8, torch.int64).view(CX, CY, WZ), "S": region(1, nb, torch.uint8),
            "reach": region(2, nb, torch.uint8), "bound": region(3, nb * 4, torch.float32), "used": region(12, nb * 32, torch.int16).view(nb, 16)}
    tabs["n_runs"] = n_runs
    tabs["n_listed"] = int((tabs["S"] == 0).sum()) * 16                 # rows left to the warp kernel (whole bricks)
    return tabs


def dqb_build_candidates(workspace, res, node_pos, knn, x_range=None):
    """Fill the per-brick candidate node lists of a dqb_workspace (what fuse_volume_dqb does itself on a call with
    rebuild_candidates=True); needed up front only by solve.sample_knn(..., bricks=...)."""
    require_gpu()
    lib = _lib.load()
    P = node_pos if isinstance(node_pos, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(node_pos, dtype=np.float64)))
    P = P.to(device="cuda", dtype=torch.float64).contiguous()
    _lib.check(lib.dfh_dqb_build_candidates(_lib.slab(res, x_range), P.data_ptr(), int(P.shape[0]), int(knn), workspace.data_ptr(),
                                            workspace.numel() * 4, current_stream_ptr()), "dfh_dqb_build_candidates")
    return workspace


def _node_tensors(node_pos, node_dq, node_w):
    def prep(a, shape_tail):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))
        t = t.to(device="cuda", dtype=torch.float64).contiguous()
        if tuple(t.shape[1:]) != shape_tail:
            raise ValueError("node array has shape %s, expected (N,%s)" % (tuple(t.shape), ",".join(map(str, shape_tail))))
        return t
    P, Q, Wn = prep(node_pos, (3,)), prep(node_dq, (8,)), prep(node_w, ())
    if not (P.shape[0] == Q.shape[0] == Wn.shape[0]):
        raise ValueError("node_pos / node_dq / node_w disagree on the number of nodes")
    return P, Q, Wn


def fuse_volume_dqb(T, Wt, live, node_pos, node_dq, node_w, knn, lw_dq, tdist, wmax=100.0, res=None,
                    x_range=None, workspace=None, rebuild_candidates=True):
    """K3 = Fusion.updateTSDF (reference core/fusion.py:153-198) on device tensors.
    node_pos (N,3), node_dq (N,8), node_w (N,) fp64 (numpy or CUDA).  `workspace` (from
    dqb_workspace) may be kept across calls; pass rebuild_candidates=False while the node
    positions, knn and slab are unchanged."""
    require_gpu()
    lib = _lib.load()
    vol, _ = _volume(T, Wt, res, x_range)
    live = _check_live(live)
    P, Q, Wn = _node_tensors(node_pos, node_dq, node_w)
    if vol.slab.x1 == vol.slab.x0:
        return T, Wt
    if workspace is None:
        workspace = dqb_workspace(vol.slab.res, (vol.slab.x0, vol.slab.x1))
        rebuild_candidates = True
    nodes = _lib.Nodes(P.data_ptr(), Q.data_ptr(), Wn.data_ptr(), int(P.shape[0]), int(knn))
    rc = lib.dfh_fuse_volume_dqb(vol, live, nodes, _lib.darr(lw_dq, 8), float(tdist), float(wmax), workspace.data_ptr(),
                                 workspace.numel() * 4, 1 if rebuild_candidates else 0, current_stream_ptr())
    _lib.check(rc, "dfh_fuse_volume_dqb")
    return T, Wt


WARPED_WEIGHTS = {"unit": 0, "node_distance": 1}                              # include/dfusion_hip.h: DFH_WARPED_W_*


def integrate_depth_dqb(T, Wt, depths, K, Kinv, lws, scale, center, tdist, node_pos, node_dq, node_w, knn, lw_dq, wmax=100.0,
                        weight="unit", tsdf_res=None, res=None, x_range=None, workspace=None, rebuild_candidates=True):
    """K1w = depth maps fused into the canonical volume through the warp field (dfh_integrate_depth_dqb): every canonical voxel
    is warped by fuse_volume_dqb's chain (Fusion.warp, reference core/fusion.py:502-551), projected into each map by
    integrate_depth's chain (core/fusion_dm.py:191-203) and the signed distance averaged in -- no live volume.
    depths: list of (H, W) CUDA tensors of one shape and dtype, lws: their 3x4 extrinsics; more than 16 views are taken 16 at a
    time.  weight: "unit" = integrate_depth's running average, "node_distance" = fuse_volume_dqb's (the mean node distance wi).
    `workspace` is a dqb_workspace, shared with fuse_volume_dqb; pass rebuild_candidates=False while the node positions, knn and
    slab are unchanged."""
    depths, lws = list(depths), list(lws)
    if len(depths) != len(lws):
        raise ValueError('length of camera matrix array must equal that of depth maps')        # core/fusion_dm.py:96-97
    if weight not in WARPED_WEIGHTS:
        raise ValueError("weight must be one of %s, not %r" % (sorted(WARPED_WEIGHTS), weight))
    batches = _view_batches(depths, lws, K, Kinv, scale, center)       # (what needs no device is checked before one is asked for)
    require_gpu()
    lib = _lib.load()
    vol, tsdf_res = _volume(T, Wt, res, x_range, tsdf_res)
    P, Q, Wn = _node_tensors(node_pos, node_dq, node_w)
    for d in depths:
        _check_depth(d)
    if vol.slab.x1 == vol.slab.x0 or not depths:
        return T, Wt
    if workspace is None:
        workspace = dqb_workspace(vol.slab.res, (vol.slab.x0, vol.slab.x1))
        rebuild_candidates = True
    nodes = _lib.Nodes(P.data_ptr(), Q.data_ptr(), Wn.data_ptr(), int(P.shape[0]), int(knn))
    for i, views in batches(tsdf_res):
        rc = lib.dfh_integrate_depth_dqb(vol, views, nodes, _lib.darr(lw_dq, 8), float(tdist), float(wmax), WARPED_WEIGHTS[weight],
                                         workspace.data_ptr(), workspace.numel() * 4, 1 if (rebuild_candidates and i == 0) else 0,
                                         current_stream_ptr())
        _lib.check(rc, "dfh_integrate_depth_dqb")
    return T, Wt


def color_volume(res, x_range=None, device=None):
    """K17: a zero-filled colour volume for planes `x_range` (default: all) of a `res` grid: float32 (x1-x0, Y, Z, 4), one
    (r, g, b, wc) pack per voxel, r g b running means in [0, 255], wc = 0: never coloured.  Always float32."""
    require_gpu()
    x0, x1 = (0, res[0]) if x_range is None else x_range
    return torch.zeros((int(x1) - int(x0), int(res[1]), int(res[2]), 4), dtype=torch.float32, device=device or "cuda")


def dqb_has_indices(workspace, res, knn, n_nodes, x_range=None):
    """True when `workspace` (a dqb_workspace) has the per-voxel node-index region that integrate_color(stored_indices=True)
    reads: the rule of dfh_integrate_depth_dqb / dfh_integrate_color."""
    lib = _lib.load()
    sl = _lib.slab(res, x_range)
    cached = lib.dfh_dqb_workspace_bytes_cached(sl, int(knn), int(n_nodes), 1)
    return cached > lib.dfh_dqb_workspace_bytes(sl) and workspace.numel() * workspace.element_size() >= cached and \
        not _lib.opt_on("k3_no_cache")


def _color_volume(C, res, x_range):
    x0, x1 = (0, res[0]) if x_range is None else x_range
    want = (int(x1) - int(x0), int(res[1]), int(res[2]), 4)
    if not (isinstance(C, torch.Tensor) and C.is_cuda and C.dtype == torch.float32 and C.is_contiguous()):
        raise ValueError("the colour volume must be a contiguous float32 CUDA tensor")
    if tuple(C.shape) != want:
        raise ValueError("colour volume shape %s does not match slab %s of grid %s" % (tuple(C.shape), want, tuple(res)))
    return _lib.ColorVolume(C.data_ptr(), _lib.slab(res, x_range))


def color_images(colors, shape=None, device=None):
    """(H, W, 3) or (H, W, 4) uint8 images (numpy or tensors) as contiguous (H, W, 4) RGBX CUDA tensors; the fourth byte is
    padding (zero when added here, kept when given).  shape: the (H, W) every image must have."""
    out = []
    for c in colors:
        t = c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c))
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] not in (3, 4):
            raise ValueError("a colour image must be (H, W, 3) or (H, W, 4) uint8")
        if shape is not None and tuple(t.shape[:2]) != tuple(shape):
            raise ValueError("colour image of %s pixels for a depth map of %s" % (tuple(t.shape[:2]), tuple(shape)))
        out.append(t)
    require_gpu()
    res = []
    for t in out:
        t = t.to(device=device or "cuda")
        if t.shape[2] == 3:
            t = torch.cat([t, torch.zeros_like(t[:, :, :1])], dim=2)
        res.append(t.contiguous())
    return res


def integrate_color(C, T, Wt, depths, colors, K, Kinv, lws, scale, center, tdist, band, node_pos=None, node_dq=None, node_w=None,
                    knn=None, lw_dq=None, wmax=100.0, band_sd=None, tsdf_res=None, res=None, x_range=None, workspace=None,
                    stored_indices=False):
    """K17 = colour images averaged into the colour volume C through the warp field (dfh_integrate_color).  Only voxels in the
    canonical band (Wt > 0, |T| <= band, T's units) are touched; such a voxel is warped by integrate_depth_dqb's chain (no nodes:
    it stays where it is), projected into each depth map, and where it lies within band_sd (depth units; default band * |scale|)
    of the measured surface the pixel's colour enters the voxel's running mean.  T, Wt are read only.
    colors: one (H, W, 3) / (H, W, 4) uint8 image per depth map.  More than 16 views are taken 16 at a time.  With nodes,
    `workspace` is a dqb_workspace whose candidate lists are current (None: one is allocated and its lists built);
    stored_indices=True reads the node indices a rebuilding fuse_volume_dqb / integrate_depth_dqb call stored in it."""
    depths, lws, colors = list(depths), list(lws), list(colors)
    if len(depths) != len(lws):
        raise ValueError('length of camera matrix array must equal that of depth maps')
    if len(colors) != len(depths):
        raise ValueError("one colour image per depth map: %d images for %d maps" % (len(colors), len(depths)))
    given = [a is not None for a in (node_pos, node_dq, node_w, knn, lw_dq)]
    if any(given) and not all(given):
        raise ValueError("node_pos, node_dq, node_w, knn and lw_dq go together")
    batches = _view_batches(depths, lws, K, Kinv, scale, center)
    if stored_indices and (not given[0] or workspace is None):
        raise ValueError("stored_indices needs nodes and the workspace that holds the indices")
    require_gpu()
    lib = _lib.load()
    vol, tsdf_res = _volume(T, Wt, res, x_range, tsdf_res)
    cvol = _color_volume(C, vol.slab.res, (vol.slab.x0, vol.slab.x1))
    for d in depths:
        _check_depth(d)
    if vol.slab.x1 == vol.slab.x0 or not depths:
        return C
    H, W = depths[0].shape
    colors = color_images(colors, (H, W), T.device)
    nodes, lw8, ws_ptr, ws_bytes = None, None, 0, 0
    if given[0]:
        P, Q, Wn = _node_tensors(node_pos, node_dq, node_w)
        if workspace is None:
            workspace = dqb_workspace(vol.slab.res, (vol.slab.x0, vol.slab.x1))
            dqb_build_candidates(workspace, vol.slab.res, P, knn, (vol.slab.x0, vol.slab.x1))
        nodes = _lib.Nodes(P.data_ptr(), Q.data_ptr(), Wn.data_ptr(), int(P.shape[0]), int(knn))
        lw8 = _lib.darr(lw_dq, 8)
        ws_ptr, ws_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    if band_sd is None:
        band_sd = float(band) * abs(float(scale))
    for i, views in batches(tsdf_res):
        cptrs = (ctypes.c_void_p * views.n_views)(*[c.data_ptr() for c in colors[i:i + 16]])
        rc = lib.dfh_integrate_color(cvol, vol, views, cptrs, nodes, lw8, float(tdist), float(band), float(band_sd), float(wmax),
                                     ws_ptr, ws_bytes, 1 if stored_indices else 0, current_stream_ptr())
        _lib.check(rc, "dfh_integrate_color")
    return C


def sample_colors(C, points, x_range=None, res=None):
    """K17: the colour volume sampled at `points` ((n, 3) fp64, global index space; numpy or CUDA), trilinear over the coloured
    corners (dfh_sample_colors): (rgb float32 (n, 3), valid bool (n,)).  C holds planes `x_range` of a grid whose first extent is
    res[0] (default: C is the whole grid)."""
    require_gpu()
    lib = _lib.load()
    if not (isinstance(C, torch.Tensor) and C.dim() == 4):
        raise ValueError("the colour volume must be a contiguous float32 CUDA tensor")
    if res is None:
        res = (C.shape[0] if x_range is None else None, C.shape[1], C.shape[2])
        if res[0] is None:
            raise ValueError("a slab's colour volume needs the grid's res")
    cvol = _color_volume(C, res, x_range)
    P = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(points, dtype=np.float64)))
    P = P.to(device=C.device, dtype=torch.float64).contiguous()
    if P.dim() != 2 or P.shape[1] != 3:
        raise ValueError("points must be (n, 3)")
    n = int(P.shape[0])
    rgb = torch.empty((n, 3), dtype=torch.float32, device=C.device)
    valid = torch.empty((n,), dtype=torch.uint8, device=C.device)
    if n:
        _lib.check(lib.dfh_sample_colors(cvol, P.data_ptr(), n, rgb.data_ptr(), valid.data_ptr(), current_stream_ptr()),
                   "dfh_sample_colors")
    return rgb, valid.bool()


def depth_prep_tile():
    """(rows, columns) of the output tile a workgroup of the depth-preprocessing kernel owns (dfh_depth_prep_tile; no launch)."""
    hw = (ctypes.c_int * 2)()
    _lib.check(_lib.load().dfh_depth_prep_tile(hw), "dfh_depth_prep_tile")
    return int(hw[0]), int(hw[1])


def depth_prep_tables(radius, sigma_s, sigma_r, n_lut=1024, cut=3.0, device=None):
    """The bilateral filter's tables for depth_prep: (spatial (2r+1, 2r+1) float32, range_lut (n_lut,) float32, range_scale), computed
    in numpy float64 and rounded to float32 (the kernel multiplies table entries; it evaluates no exp):
      spatial[dy][dx] = exp(-(dx^2 + dy^2) / (2 sigma_s^2))
      range_scale     = float32(n_lut / (cut * sigma_r)^2)       a squared depth difference times it is the LUT index; differences
                                                                 beyond cut * sigma_r fall off the table and do not count
      range_lut[i]    = exp(-((i + 0.5) / range_scale) / (2 sigma_r^2))
    sigma_s in pixels, sigma_r in the depth maps' units.  device: default the current GPU ("cpu" gives host tensors)."""
    radius, n_lut = int(radius), int(n_lut)
    if not 0 <= radius <= 8:
        raise ValueError("radius must be 0..8, got %d" % radius)
    if not 1 <= n_lut <= 4096:
        raise ValueError("n_lut must be 1..4096, got %d" % n_lut)
    if not (sigma_s > 0 and sigma_r > 0 and cut > 0):
        raise ValueError("sigma_s, sigma_r and cut must be positive")
    o = np.arange(-radius, radius + 1, dtype=np.float64)
    spatial = np.exp(-(o[None, :] ** 2 + o[:, None] ** 2) / (2.0 * float(sigma_s) ** 2)).astype(np.float32)
    range_scale = float(np.float32(n_lut / (float(cut) * float(sigma_r)) ** 2))
    lut = np.exp(-((np.arange(n_lut, dtype=np.float64) + 0.5) / range_scale) / (2.0 * float(sigma_r) ** 2)).astype(np.float32)
    if device is None:
        require_gpu()
        device = torch.device("cuda", torch.cuda.current_device())
    return torch.from_numpy(spatial).to(device), torch.from_numpy(lut).to(device), range_scale


def depth_prep(depths, Kinv, tables, max_jump, min_cos, mask=True, want_normals=True, out=None):
    """K12 = the frame's depth maps filtered, given normals and masked in one launch (dfh_depth_prep; semantics in
    include/dfusion_hip.h).  depths: list of at most 16 (H, W) CUDA tensors of one shape and dtype (float32 / float64), only read.
    tables: depth_prep_tables(...) on the maps' device; the window radius is the spatial table's.  max_jump: largest depth step
    between neighbours a normal is computed across; min_cos: smallest cosine between the normal and the viewing ray.
    Returns (clean (V, H, W) float32, normals (V, H, W, 3) float32 or None): clean[v] is a depth map every other entry point
    reads (negative depth, 0 = no measurement); with mask=True the pixels without a normal are 0 in it.
    out=(clean, normals): write into these tensors instead of fresh ones (either may be None: that output is not produced).  The
    kernel writes through raw pointers, so the tensors' version counters are bumped here: whatever keys a cache on
    (data_ptr, _version), WarpSolver's packed views table for one, sees new content."""
    depths = list(depths)
    if not depths:
        raise ValueError("depth_prep needs at least one depth map")
    if len(depths) > 16:
        raise ValueError("at most 16 depth maps per call, got %d" % len(depths))
    for d in depths:
        if not (isinstance(d, torch.Tensor) and d.dim() == 2):
            raise ValueError("depth must be a contiguous 2-D CUDA tensor")
        if d.shape != depths[0].shape or d.dtype != depths[0].dtype:
            raise ValueError("all depth maps of one call must have the same shape and dtype")
    spatial, range_lut, range_scale = tables
    if spatial.dim() != 2 or spatial.shape[0] != spatial.shape[1] or spatial.shape[0] % 2 != 1:
        raise ValueError("spatial table must be (2r+1, 2r+1), got %s" % (tuple(spatial.shape),))
    side = int(spatial.shape[0])
    for t in (spatial, range_lut):
        if not (t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("filter tables must be contiguous float32 tensors")
    require_gpu()
    lib = _lib.load()
    for d in depths:
        _check_depth(d)
    dev = depths[0].device
    if spatial.device != dev or range_lut.device != dev:
        raise ValueError("filter tables must live on the depth maps' device")
    V = len(depths)
    H, W = (int(n) for n in depths[0].shape)
    if out is None:
        clean = torch.empty((V, H, W), dtype=torch.float32, device=dev)
        normals = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev) if want_normals else None
    else:
        clean, normals = out
        for t, shape in ((clean, (V, H, W)), (normals, (V, H, W, 3))):
            if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and
                                      t.is_contiguous() and tuple(t.shape) == shape):
                raise ValueError("out tensor must be a contiguous float32 CUDA tensor of shape %s" % (shape,))
    ptrs = (ctypes.c_void_p * V)(*[d.data_ptr() for d in depths])
    prm = _lib.DepthPrepParams(V, ptrs, dtype_code(depths[0]), H, W, _lib.darr(Kinv, 9), (side - 1) // 2, spatial.data_ptr(),
                               range_lut.data_ptr(), int(range_lut.numel()), float(range_scale), float(max_jump), float(min_cos),
                               1 if mask else 0)
    rc = lib.dfh_depth_prep(prm, None if clean is None else clean.data_ptr(), None if normals is None else normals.data_ptr(),
                            current_stream_ptr())
    _lib.check(rc, "dfh_depth_prep")
    if out is not None:
        torch.autograd.graph.increment_version(tuple(t for t in (clean, normals) if t is not None))
    return clean, normals


def rgbd_ingest_tile():
    """(rows, columns) of the output tile a workgroup of the RGB-D ingest kernels owns (dfh_rgbd_ingest_tile; no launch)."""
    hw = (ctypes.c_int * 2)()
    _lib.check(_lib.load().dfh_rgbd_ingest_tile(hw), "dfh_rgbd_ingest_tile")
    return int(hw[0]), int(hw[1])


def rgbd_ingest_workspace(n_views, Hc, Wc, device=None):
    """The workspace of one rgbd_ingest call with colour: an int32 tensor of dfh_rgbd_ingest_workspace_bytes(); its first
    n_views * Hc * Wc elements are the colour camera's z-buffer after the call (rgbd_ingest returns that view)."""
    nbytes = _lib.load().dfh_rgbd_ingest_workspace_bytes(int(n_views), int(Hc), int(Wc))
    if nbytes == 0:
        raise ValueError("bad z-buffer size: %d views of %d x %d" % (n_views, Hc, Wc))
    return torch.empty((nbytes + 7) // 8 * 2, dtype=torch.int32, device=device or "cuda")


RGBD_SAMPLE = {"nearest": 0, "bilinear": 1}


def rgbd_ingest(raw_depths, raw_colors, views, out_intrinsics, depth_scale=1e-3, z_min=0.0, z_max=0.0, occl_tol=0.0, max_splat=8,
                sample="bilinear", want_color_depth=True, out=None, workspace=None):
    """K19 = raw sensor frames to frame inputs in at most three launches (dfh_rgbd_ingest; semantics in include/dfusion_hip.h).
    raw_depths: list of at most 16 (Hd, Wd) uint16 CUDA tensors (torch.uint16, or int16 holding the same bits), only read.
    raw_colors: None, or one (Hc, Wc, 3) / (Hc, Wc, 4) uint8 CUDA tensor per depth map.  views: one record per map,
    (fd[4], kd[5], fc[4], kc[5], T_dc[12]) -- 30 numbers, or a 5-tuple of those arrays -- or a ready (_lib.RGBDView * V) array.  out_intrinsics: (fx, fy, cx, cy) of the
    pinhole the output maps are resampled to.
    Returns (depth (V, Hd, Wd) float32, color (V, Hd, Wd, 4) uint8 or None, color_depth (V, Hd, Wd) float32 or None,
    zbuf (V, Hc, Wc) int32 view of the workspace or None).
    out=(depth, color, color_depth): write into these tensors instead of fresh ones (color_depth may be None: not produced).  The
    kernels write through raw pointers, so the tensors' version counters are bumped here, as depth_prep does.
    workspace: an rgbd_ingest_workspace(V, Hc, Wc) to reuse (default: a fresh one)."""
    raw_depths = list(raw_depths)
    V = len(raw_depths)
    if V == 0:
        raise ValueError("rgbd_ingest needs at least one depth map")
    if V > 16:
        raise ValueError("at most 16 views per call, got %d" % V)
    u16 = tuple(t for t in (getattr(torch, "uint16", None), torch.int16) if t is not None)
    for d in raw_depths:
        if not (isinstance(d, torch.Tensor) and d.dim() == 2 and d.dtype in u16):
            raise ValueError("a raw depth map must be a contiguous 2-D 16-bit integer CUDA tensor")
        if d.shape != raw_depths[0].shape:
            raise ValueError("all raw depth maps of one call must have the same shape")
    colour = raw_colors is not None
    if colour:
        raw_colors = list(raw_colors)
        if len(raw_colors) != V:
            raise ValueError("one colour image per depth map: %d images for %d maps" % (len(raw_colors), V))
        for c in raw_colors:
            if not (isinstance(c, torch.Tensor) and c.dim() == 3 and c.dtype == torch.uint8 and c.shape[2] in (3, 4)):
                raise ValueError("a raw colour image must be a contiguous (H, W, 3) or (H, W, 4) uint8 CUDA tensor")
            if c.shape != raw_colors[0].shape:
                raise ValueError("all raw colour images of one call must have the same shape")
    if sample not in RGBD_SAMPLE:
        raise ValueError("sample must be one of %s, not %r" % (sorted(RGBD_SAMPLE), sample))
    if not (isinstance(views, ctypes.Array) and getattr(views, "_type_", None) is _lib.RGBDView):
        views = list(views)
    if len(views) != V:
        raise ValueError("one calibration record per depth map: %d records for %d maps" % (len(views), V))
    prepacked = isinstance(views, ctypes.Array) and getattr(views, "_type_", None) is _lib.RGBDView
    recs = views if prepacked else (_lib.RGBDView * V)()
    for r, v in zip(recs, () if prepacked else views):
        a = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in v]) if isinstance(v, (tuple, list)) and len(v) == 5 \
            else np.asarray(v, dtype=np.float64).reshape(-1)
        if a.size != 30:
            raise ValueError("a calibration record is fd[4], kd[5], fc[4], kc[5], T_dc[12]: 30 numbers, got %d" % a.size)
        ctypes.memmove(ctypes.byref(r), np.ascontiguousarray(a).ctypes.data, 240)
    fx, fy, cx, cy = (float(x) for x in np.asarray(out_intrinsics, dtype=np.float64).reshape(-1))
    require_gpu()
    lib = _lib.load()
    for t in raw_depths + (raw_colors if colour else []):
        if not (t.is_cuda and t.is_contiguous()):
            raise ValueError("raw maps and images must be contiguous CUDA tensors")
    dev = raw_depths[0].device
    Hd, Wd = (int(n) for n in raw_depths[0].shape)
    Hc, Wc, C = (int(n) for n in raw_colors[0].shape) if colour else (0, 0, 0)
    if out is None:
        depth = torch.empty((V, Hd, Wd), dtype=torch.float32, device=dev)
        color = torch.empty((V, Hd, Wd, 4), dtype=torch.uint8, device=dev) if colour else None
        cdepth = torch.empty((V, Hd, Wd), dtype=torch.float32, device=dev) if colour and want_color_depth else None
    else:
        depth, color, cdepth = out
        for t, shape, dt in ((depth, (V, Hd, Wd), torch.float32), (color, (V, Hd, Wd, 4), torch.uint8), (cdepth, (V, Hd, Wd), torch.float32)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dt and t.is_contiguous() and
                                      tuple(t.shape) == shape):
                raise ValueError("out tensor must be a contiguous %s CUDA tensor of shape %s" % (dt, shape))
        if depth is None or (colour and color is None):
            raise ValueError("out needs a depth tensor, and a color tensor when colour images are given")
        if not colour:
            color = cdepth = None
    zbuf = None
    if colour:
        nbytes = lib.dfh_rgbd_ingest_workspace_bytes(V, Hc, Wc)
        if workspace is None:
            workspace = rgbd_ingest_workspace(V, Hc, Wc, dev)
        elif not (isinstance(workspace, torch.Tensor) and workspace.device == dev and workspace.is_contiguous() and
                  workspace.numel() * workspace.element_size() >= nbytes):
            raise ValueError("workspace must be a contiguous CUDA tensor of at least %d bytes" % nbytes)
        zbuf = workspace.view(torch.int32)[:V * Hc * Wc].view(V, Hc, Wc)
    dptrs = (ctypes.c_void_p * V)(*[d.data_ptr() for d in raw_depths])
    cptrs = (ctypes.c_void_p * V)(*[c.data_ptr() for c in raw_colors]) if colour else None
    prm = _lib.RGBDIngestParams(V, dptrs, cptrs, Hd, Wd, Hc, Wc, C, fx, fy, cx, cy, float(depth_scale), float(z_min), float(z_max),
                                float(occl_tol), int(max_splat), RGBD_SAMPLE[sample], recs)
    rc = lib.dfh_rgbd_ingest(prm, depth.data_ptr(), None if color is None else color.data_ptr(),
                             None if cdepth is None else cdepth.data_ptr(), None if workspace is None or not colour else workspace.data_ptr(),
                             current_stream_ptr())
    _lib.check(rc, "dfh_rgbd_ingest")
    if out is not None:
        torch.autograd.graph.increment_version(tuple(t for t in (depth, color, cdepth) if t is not None))
    return depth, color, cdepth, zbuf


def raycast_table(T, res=None, x_range=None, out=None):
    """K20: the brick table that lets raycast step over empty space (dfh_raycast_table): one uint8 per 8 x 8 x 8-cell brick of the
    slab T holds, 1 = live (some voxel of the brick or of the one-voxel ring around it is not safely > 0), 0 = dead.  The table
    describes T as it is NOW: rebuild it after T changes.  out: a uint8 CUDA tensor of at least the table's size to fill."""
    if not (isinstance(T, torch.Tensor) and T.is_cuda and T.is_contiguous() and T.dim() == 3 and T.dtype in (torch.float32, torch.float64)):
        raise ValueError("the volume must be a contiguous 3-D float32 or float64 CUDA tensor")
    require_gpu()
    lib = _lib.load()
    vol, _ = _volume(T, T, res, x_range)
    n = lib.dfh_raycast_table_bytes(vol.slab)
    if out is None:
        out = torch.empty((n,), dtype=torch.uint8, device=T.device)
    elif not (isinstance(out, torch.Tensor) and out.device == T.device and out.dtype == torch.uint8 and out.is_contiguous() and
              out.numel() >= n):
        raise ValueError("out must be a contiguous uint8 CUDA tensor of at least %d elements" % n)
    if n:
        _lib.check(lib.dfh_raycast_table(vol, out.data_ptr(), current_stream_ptr()), "dfh_raycast_table")
        torch.autograd.graph.increment_version((out,))
    return out


def raycast_inverse_views(lws):
    """The camera -> world 3 x 4 matrices raycast passes beside `lws` (world -> camera 3 x 4 each): wl = [R^-1 | -R^-1 t], in
    numpy float64.  The device inverts nothing; a caller that needs exact matrices passes its own through raycast(wls=)."""
    out = []
    for lw in lws:
        m = np.asarray(lw, dtype=np.float64).reshape(3, 4)
        ri = np.linalg.inv(m[:, :3])
        out.append(np.concatenate([ri, -(ri @ m[:, 3:])], axis=1))
    return out


class RaycastResult:
    """What raycast returns: .depth (V, H, W) float32 (negative depth, 0 = miss), .normals (V, H, W, 3) float32 (camera space,
    facing the camera, zeros = none), .color (V, H, W, 4) uint8 (RGBX, X = 255 where valid), .hit (V, H, W, 3) float32 (index
    space, NaN = miss); the ones not asked for are None."""
    __slots__ = ("depth", "normals", "color", "hit")

    def __init__(self, depth=None, normals=None, color=None, hit=None):
        self.depth, self.normals, self.color, self.hit = depth, normals, color, hit


# raycast_skip = -1, "the library decides": a call without a table builds one where the table build plus the skipping march
# beat the plain march by more than the spread of either (profiles/r21_raycast.txt: measured at 256^3 with 3 x 640x480 rays and
# at 512^3 with 8 x 1280x720).  Smaller volumes or fewer rays have not been measured: they march plainly.
RAYCAST_SKIP_MIN_VOXELS = 256 ** 3
RAYCAST_SKIP_MIN_RAYS = 640 * 480


def raycast_builds_table(option, n_voxels, n_rays):
    """Whether a raycast call that was given no table builds one: option raycast_skip 1 = always, 0 = never, -1 = by size."""
    if option == 1:
        return True
    return option < 0 and n_voxels >= RAYCAST_SKIP_MIN_VOXELS and n_rays >= RAYCAST_SKIP_MIN_RAYS


RAYCAST_OUTPUTS = {"depth": ((), torch.float32), "normals": ((3,), torch.float32), "color": ((4,), torch.uint8),
                   "hit": ((3,), torch.float32)}


def raycast(T, Wt, K, Kinv, lws, H, W, scale, center, tsdf_res=None, res=None, x_range=None, step=0.5, z_near=0.0, z_far=float("inf"),
            min_weight=0.0, refine=1, max_steps=1 << 20, colors=None, table=None, want=("depth", "normals"), out=None, wls=None):
    """K20 = the volume (T, Wt) seen from the cameras `lws` (world -> camera 3 x 4 each, any number: 16 per launch) through K:
    a ray per pixel marched in steps of `step` voxels to the first + to - crossing of the trilinear TSDF, refined by `refine`
    secant steps (dfh_raycast; semantics in include/dfusion_hip.h).  A sample counts only where all eight corners have
    Wt >= min_weight (0: Wt is not read).  want: which of "depth", "normals", "color", "hit" to produce; "color" needs `colors`,
    the slab's colour volume.  table: a raycast_table(T) to skip empty space with (same bits), the caller's to cache while T does
    not change; None builds one here where that pays (raycast_builds_table: option raycast_skip 1 always, 0 never -- and a
    given table is ignored --, unset by size) and marches plainly otherwise.  out: a RaycastResult whose tensors are written instead of fresh ones.
    wls: the exact camera -> world matrices, if the caller has them (default raycast_inverse_views(lws)).  T, Wt, colors: only read."""
    lws = list(lws)
    V = len(lws)
    if V == 0:
        raise ValueError("raycast needs at least one view")
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in RAYCAST_OUTPUTS for w in want):
        raise ValueError("want must name some of %s, not %r" % (sorted(RAYCAST_OUTPUTS), want))
    if "color" in want and colors is None:
        raise ValueError("color wanted without a colour volume")
    if wls is None:
        wls = raycast_inverse_views(lws)
    wls = list(wls)
    if len(wls) != V:
        raise ValueError("one inverse per view: %d for %d views" % (len(wls), V))
    H, W = int(H), int(W)
    require_gpu()
    lib = _lib.load()
    vol, tsdf_res = _volume(T, Wt, res, x_range, tsdf_res)
    xr = (vol.slab.x0, vol.slab.x1)
    cvol = _color_volume(colors, vol.slab.res, xr) if colors is not None else None
    skip = _lib.get_option("raycast_skip")
    n_vox = (xr[1] - xr[0]) * vol.slab.res[1] * vol.slab.res[2]
    if table is None and n_vox and raycast_builds_table(skip, n_vox, V * H * W):
        table = raycast_table(T, tuple(vol.slab.res), xr)
    if table is not None and not (isinstance(table, torch.Tensor) and table.device == T.device and table.dtype == torch.uint8 and
                                  table.is_contiguous()):
        raise ValueError("table must be a contiguous uint8 CUDA tensor (raycast_table)")
    result = RaycastResult() if out is None else out
    for name in want:
        tail, dt = RAYCAST_OUTPUTS[name]
        t = getattr(result, name)
        if t is None:
            setattr(result, name, torch.empty((V, H, W) + tail, dtype=dt, device=T.device))
        elif not (isinstance(t, torch.Tensor) and t.device == T.device and t.dtype == dt and t.is_contiguous() and
                  tuple(t.shape) == (V, H, W) + tail):
            raise ValueError("out.%s must be a contiguous %s CUDA tensor of shape %s" % (name, dt, (V, H, W) + tail))
    cen = _lib.darr(np.asarray(center, dtype=np.float64), 3)
    for i in range(0, V, 16):
        n = min(16, V - i)
        lw = _lib.darr(np.concatenate([np.asarray(l, dtype=np.float64).reshape(12) for l in lws[i:i + n]]), 12 * n)
        wl = _lib.darr(np.concatenate([np.asarray(l, dtype=np.float64).reshape(12) for l in wls[i:i + n]]), 12 * n)
        ptr = {}
        for name in RAYCAST_OUTPUTS:
            t = getattr(result, name) if name in want else None
            ptr[name] = None if t is None else t.data_ptr() + i * t.stride(0) * t.element_size()
        prm = _lib.RaycastParams(ctypes.pointer(vol), None if cvol is None else ctypes.pointer(cvol), n, H, W, _lib.darr(K, 9),
                                 _lib.darr(Kinv, 9), lw, wl, float(scale), cen, float(tsdf_res) / 2.0, float(z_near), float(z_far),
                                 float(step), float(min_weight), int(refine), int(max_steps),
                                 None if table is None else table.data_ptr(), 0 if table is None else table.numel(),
                                 ptr["depth"], ptr["normals"], ptr["color"], ptr["hit"])
        _lib.check(lib.dfh_raycast(prm, current_stream_ptr()), "dfh_raycast")
    if out is not None:
        torch.autograd.graph.increment_version(tuple(getattr(result, name) for name in want))
    return result


def depth_halve(depths, max_jump, out=None):
    """K21 = one step of the depth pyramid for all maps of a frame in one launch (dfh_depth_halve; semantics in
    include/dfusion_hip.h): every output pixel is the mean of the valid taps of its 2 x 2 block that lie within max_jump of the
    block's first pixel, 0 where that pixel holds no measurement.  depths: a (V, H, W) CUDA tensor or a list of at most 16
    (H, W) CUDA tensors of one shape and dtype (float32 / float64), only read.  Returns (V, H // 2, W // 2) float32."""
    depths = list(depths)
    if not depths:
        raise ValueError("depth_halve needs at least one depth map")
    if len(depths) > 16:
        raise ValueError("at most 16 depth maps per call, got %d" % len(depths))
    for d in depths:
        if not (isinstance(d, torch.Tensor) and d.dim() == 2):
            raise ValueError("depth must be a contiguous 2-D CUDA tensor")
        if d.shape != depths[0].shape or d.dtype != depths[0].dtype:
            raise ValueError("all depth maps of one call must have the same shape and dtype")
    require_gpu()
    lib = _lib.load()
    for d in depths:
        _check_depth(d)
    V = len(depths)
    H, W = (int(n) for n in depths[0].shape)
    dev = depths[0].device
    shape = (V, H // 2, W // 2)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.device == dev and out.dtype == torch.float32 and out.is_contiguous() and
              tuple(out.shape) == shape):
        raise ValueError("out must be a contiguous float32 CUDA tensor of shape %s" % (shape,))
    ptrs = (ctypes.c_void_p * V)(*[d.data_ptr() for d in depths])
    _lib.check(lib.dfh_depth_halve(ptrs, V, dtype_code(depths[0]), H, W, float(max_jump), out.data_ptr(), current_stream_ptr()),
               "dfh_depth_halve")
    torch.autograd.graph.increment_version((out,))
    return out


def icp_track_scratch(n_views, device=None):
    """The workspace of icp_track for n_views views (dfh_icp_track_bytes; no initial state, reusable across calls)."""
    require_gpu()
    n = int(_lib.load().dfh_icp_track_bytes(int(n_views)))
    if n == 0:
        raise ValueError("icp_track takes 1..16 views per call, got %d" % n_views)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return torch.empty(n // 8, dtype=torch.float64, device=device)


def icp_track(live_depth, live_normals, model_depth, model_normals, K, Kinv, T, n_iters, max_dist=0.0, min_cos=0.0, huber=0.0,
              lm_rel=0.0, min_count=6, max_rot=float("inf"), max_trans=float("inf"), want_rows=False, scratch=None):
    """K21 = n_iters iterations of dense projective point-to-plane ICP for all views of one pyramid level (dfh_icp_track; semantics
    in include/dfusion_hip.h), queued back to back: nothing is read back.  live_depth, model_depth: (V, H, W) float32 CUDA;
    model_normals, live_normals: (V, H, W, 3) float32 CUDA (live_normals None: no normal gate).  T: (V, 3, 4) float64 CUDA, live
    camera -> model camera, updated IN PLACE.  Returns (stats (V, n_iters, 40) float64: 29 sums | status | xi | 0, rows
    (V, H, W, 8) float64 of the first iteration or None)."""
    require_gpu()
    lib = _lib.load()
    if not (isinstance(live_depth, torch.Tensor) and live_depth.dim() == 3 and live_depth.is_cuda):
        raise ValueError("live_depth must be a (V, H, W) CUDA tensor")
    V, H, W = (int(n) for n in live_depth.shape)
    dev = live_depth.device
    for name, t, shape in (("live_depth", live_depth, (V, H, W)), ("model_depth", model_depth, (V, H, W)),
                           ("model_normals", model_normals, (V, H, W, 3)), ("live_normals", live_normals, (V, H, W, 3))):
        if t is None and name == "live_normals":
            continue
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and
                tuple(t.shape) == shape):
            raise ValueError("%s must be a contiguous float32 CUDA tensor of shape %s" % (name, shape))
    if not (isinstance(T, torch.Tensor) and T.device == dev and T.dtype == torch.float64 and T.is_contiguous() and
            tuple(T.shape) == (V, 3, 4)):
        raise ValueError("T must be a contiguous float64 CUDA tensor of shape %s" % ((V, 3, 4),))
    n_iters = int(n_iters)
    if not 0 <= n_iters <= 64:
        raise ValueError("n_iters must be 0..64, got %d" % n_iters)
    if scratch is None:
        scratch = icp_track_scratch(V, dev)
    if not (isinstance(scratch, torch.Tensor) and scratch.device == dev and scratch.is_contiguous()):
        raise ValueError("scratch must be a contiguous CUDA tensor (icp_track_scratch)")
    stats = torch.empty((V, n_iters, 40), dtype=torch.float64, device=dev)
    rows = torch.empty((V, H, W, 8), dtype=torch.float64, device=dev) if want_rows and n_iters > 0 else None
    prm = _lib.IcpTrackParams(V, H, W, live_depth.data_ptr(), None if live_normals is None else live_normals.data_ptr(),
                              model_depth.data_ptr(), model_normals.data_ptr(), _lib.darr(K, 9), _lib.darr(Kinv, 9), T.data_ptr(),
                              float(max_dist), float(min_cos), float(huber), float(lm_rel), n_iters, int(min_count), float(max_rot),
                              float(max_trans), stats.data_ptr() if n_iters else None, None if rows is None else rows.data_ptr(),
                              scratch.data_ptr(), scratch.numel() * scratch.element_size())
    _lib.check(lib.dfh_icp_track(prm, current_stream_ptr()), "dfh_icp_track")
    if n_iters:
        torch.autograd.graph.increment_version((T,))
    return stats, rows
