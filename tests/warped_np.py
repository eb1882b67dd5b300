"""numpy restatement of dfh_integrate_depth_dqb (K1w) and the scenes its tests share.

The restatement composes the oracle's own pieces: oracle_np.knn_bruteforce and oracle_np.warp (Fusion.warp) for the warped
position of every canonical voxel, then the projection lines of oracle_np.fuse_depths with the voxel index replaced by that
position, then one of the two running averages.  Beside the updated volumes it returns, per view, the update mask and, per
voxel, the distance to every decision boundary of the chain, so that a GPU comparison can leave out (and count) the voxels
whose decision hangs on the last ulp of exp() or of a division:
  pixel : distance of u or v to a .5-pixel tie of round()                  (pixels)
  edge  : distance of u or v to a frustum edge 0, W-1, H-1                 (pixels)
  sd    : |sd + tdist| where the view has a measurement                    (depth units)
  tie   : distance of an inner-warp coordinate to a float32 rounding tie   (float32 ulps)
"""
import numpy as np

from oracle import oracle_np as O

IDENT = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])

# the exclusion rule of the GPU-against-numpy comparisons
TIE_ULP, PIXEL_PX, SD_M = 1e-4, 1e-6, 1e-9
MAX_EXCLUDED = 0.005


def f32_tie_distance(v):
    """Distance of each double to the nearest float32 rounding tie, in float32 ulps of its binade."""
    v = np.asarray(v, dtype=np.float64)
    f = v.astype(np.float32)
    ulp = np.spacing(np.abs(f)).astype(np.float64)
    return np.abs(0.5 - np.abs(v - f.astype(np.float64)) / ulp)


def integrate_depth_dqb_np(T, Wt, depths, lws, K, Kinv, scale, center, tdist, node_pos, node_dq, node_w, knn, lw_dq,
                           wmax=100.0, weight="unit", tsdf_res=None, x_range=None, chunk=4):
    """In place on T / Wt (any float dtype: arithmetic is fp64, rounded to the arrays' dtype after every view).
    Returns (T, Wt, masks (V, *T.shape) bool, margins dict of T.shape arrays)."""
    node_pos = np.asarray(node_pos, dtype=np.float64)
    node_dq = np.asarray(node_dq, dtype=np.float64)
    node_w = np.asarray(node_w, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64)
    Kinv = np.asarray(Kinv, dtype=np.float64)
    center = np.asarray(center, dtype=np.float64)
    X, Y, Z = T.shape
    a, b = (0, T.shape[0]) if x_range is None else x_range
    assert b - a == T.shape[0]
    c = (X if tsdf_res is None else tsdf_res) / 2
    V = len(depths)
    masks = np.zeros((V,) + T.shape, dtype=bool)
    big = np.inf
    margins = {k: np.full(T.shape, big) for k in ("pixel", "edge", "sd", "tie")}
    for s in range(a, b, chunk):
        e = min(b, s + chunk)
        sl = slice(s - a, e - a)
        ix, iy, iz = O._voxel_index_grid((b, Y, Z), s, e)
        pos = np.stack(np.broadcast_arrays(ix, iy, iz), axis=-1)
        loc = O.knn_bruteforce(pos, node_pos, knn)
        q = O.warp(pos, node_dq[loc], node_pos[loc], node_w[loc], m_lw=lw_dq)
        x1 = O.dqb_warp(O.dq_blend(pos, node_dq[loc], node_pos[loc], node_w[loc]), pos)      # the inner warp's output
        margins["tie"][sl] = np.min(f32_tie_distance(x1), axis=-1)
        wi = np.zeros(pos.shape[:-1])
        for j in range(knn):
            wi = wi + O._norm3(node_pos[loc[..., j]] - pos) / knn
        for v in range(V):
            dm, lw = np.asarray(depths[v]), np.asarray(lws[v], dtype=np.float64)
            H, W = dm.shape
            px = scale * (q[..., 0] - c) + center[0]
            py = scale * (q[..., 1] - c) + center[1]
            pz = scale * (q[..., 2] - c) + center[2]
            l0 = lw[0, 0] * px + lw[0, 1] * py + lw[0, 2] * pz + lw[0, 3]
            l1 = lw[1, 0] * px + lw[1, 1] * py + lw[1, 2] * pz + lw[1, 3]
            l2 = lw[2, 0] * px + lw[2, 1] * py + lw[2, 2] * pz + lw[2, 3]
            p0 = K[0, 0] * l0 + K[0, 1] * l1 + K[0, 2] * l2
            p1 = K[1, 0] * l0 + K[1, 1] * l1 + K[1, 2] * l2
            p2 = K[2, 0] * l0 + K[2, 1] * l1 + K[2, 2] * l2
            ok = p2 != 0
            p2s = np.where(ok, p2, 1.0)
            u = p0 / p2s
            vv = p1 / p2s
            vis = ok & (u >= 0) & (u < W - 1) & (vv >= 0) & (vv < H - 1)
            ui = np.where(vis, np.rint(u), 0).astype(np.int64)
            vi = np.where(vis, np.rint(vv), 0).astype(np.int64)
            z = -1 * dm[vi, ui].astype(np.float64)
            val = vis & (z > 0)
            with np.errstate(invalid="ignore", over="ignore"):
                cz = Kinv[2, 0] * (z * u) + Kinv[2, 1] * (z * vv) + Kinv[2, 2] * (z * 1.0)
                sd = cz - l2
                upd = val & (sd > -1 * tdist)
            m = np.minimum(np.abs(u - np.floor(u) - 0.5), np.abs(vv - np.floor(vv) - 0.5))
            margins["pixel"][sl] = np.minimum(margins["pixel"][sl], np.where(vis, m, big))
            edge = np.minimum(np.minimum(np.abs(u), np.abs(u - (W - 1))), np.minimum(np.abs(vv), np.abs(vv - (H - 1))))
            margins["edge"][sl] = np.minimum(margins["edge"][sl], np.where(ok, edge, big))
            with np.errstate(invalid="ignore"):
                msd = np.where(val & np.isfinite(sd), np.abs(sd + tdist), big)
            margins["sd"][sl] = np.minimum(margins["sd"][sl], msd)
            Tv = T[sl].astype(np.float64)
            W0 = Wt[sl].astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                if weight == "unit":
                    newT = (scale * Tv * W0 + np.minimum(tdist, sd)) / (scale * (1 + W0))
                    newW = np.minimum(1 + W0, wmax)
                else:
                    Wv = np.where(W0 == 0, wi, W0)
                    newT = (Tv * Wv + (np.minimum(tdist, sd) / scale) * wi) / (wi + Wv)
                    newW = np.minimum(wi + Wv, wmax)
            T[sl] = np.where(upd, newT, Tv)
            Wt[sl] = np.where(upd, newW, W0)
            masks[v][sl] = upd
    return T, Wt, masks, margins


def excluded(margins):
    """The voxels the exclusion rule leaves out of a GPU-against-numpy comparison."""
    return (margins["tie"] < TIE_ULP) | (margins["pixel"] < PIXEL_PX) | (margins["edge"] < PIXEL_PX) | (margins["sd"] < SD_M)


# ---------------------------------------------------------------------------------------------- scenes
def small_dq(rng, rot, trans, dscale):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(-rot, rot)
    q = np.append(np.cos(ang / 2), np.sin(ang / 2) * ax)
    t = rng.uniform(-trans, trans, size=3)
    qe = 0.5 * O.quaternion_multiply(np.array([0.0, t[0], t[1], t[2]]), q)
    return np.append(q, qe) * (1.0 + rng.uniform(-dscale, dscale))


def field(rng, n, rot=0.06, trans=0.5, dscale=0.02):
    """Per-node random rotations up to `rot` rad, translations up to `trans` voxel, DQ scale 1 +- dscale."""
    return np.stack([small_dq(rng, rot, trans, dscale) for _ in range(n)])


def camera(res, angles=(0.0, 40.0), name="C1", dtype=np.float32):
    """(K, Kinv, depths, lws, scale, center, tdist) of scene's sphere-and-wall seen from `angles` on a res^3 grid."""
    from dynamicfusion_body_amd import scene
    H, W, fx, cx, cy = scene.CAMERAS[name]
    K = scene.intrinsics(fx, cx, cy)
    scale, center, tdist = scene.grid_params(res)
    lws = [scene.view_extrinsic(a) for a in angles]
    depths = [scene.render_depth(K, lw, H, W, dtype=dtype) for lw in lws]
    return K, np.linalg.inv(K), depths, lws, scale, center, tdist


def main_scene(knn_nodes=48, res=32, seed=11):
    """The main scene: res 32, camera C1, views at 0 and 40 degrees, 48 Fibonacci nodes with a non-rigid field and a small
    non-identity lw_dq; volumes start at (tdist / scale, 0)."""
    from dynamicfusion_body_amd import scene
    K, Kinv, depths, lws, scale, center, tdist = camera(res)
    node_pos, node_w = scene.fibonacci_nodes(knn_nodes, res)
    rng = np.random.default_rng(seed)
    node_dq = field(rng, knn_nodes)
    lw_dq = small_dq(rng, 0.01, 0.1, 0.0)
    return dict(K=K, Kinv=Kinv, depths=depths, lws=lws, scale=scale, center=center, tdist=tdist, node_pos=node_pos, node_w=node_w,
                node_dq=node_dq, lw_dq=lw_dq, shape=(res, res, res), tsdf_res=res)


def ragged_scene(seed=5):
    """(13, 11, 21) voxels of a tsdf_res = 21 grid, 40 random nodes."""
    K, Kinv, depths, lws, scale, center, tdist = camera(21)
    shape = (13, 11, 21)
    rng = np.random.default_rng(seed)
    node_pos = rng.uniform(0, 1, size=(40, 3)) * np.array(shape)
    node_w = np.full(40, 6.0)
    node_dq = field(rng, 40)
    lw_dq = small_dq(rng, 0.01, 0.1, 0.0)
    return dict(K=K, Kinv=Kinv, depths=depths, lws=lws, scale=scale, center=center, tdist=tdist, node_pos=node_pos, node_w=node_w,
                node_dq=node_dq, lw_dq=lw_dq, shape=shape, tsdf_res=21)


def clustered_scene(seed=9):
    """320 nodes clustered at the grid centre of a 16 x 16 x 32 slab of a 32^3 grid's frame (more than the 256 candidates a
    brick keeps: the device scans every node), plus 40 spread out."""
    K, Kinv, depths, lws, scale, center, tdist = camera(32)
    shape = (16, 16, 32)
    rng = np.random.default_rng(seed)
    node_pos = rng.uniform(0, 1, size=(360, 3)) * np.array(shape)
    node_pos[:320] = np.array(shape) / 2.0 + rng.normal(size=(320, 3)) * 1.5
    node_w = np.full(360, 5.0)
    node_dq = field(rng, 360)
    lw_dq = small_dq(rng, 0.01, 0.1, 0.0)
    return dict(K=K, Kinv=Kinv, depths=depths, lws=lws, scale=scale, center=center, tdist=tdist, node_pos=node_pos, node_w=node_w,
                node_dq=node_dq, lw_dq=lw_dq, shape=shape, tsdf_res=32)


def skewed(K):
    """K with a skew and a projective row, and its inverse, whose third row is full: the general projection chain."""
    K = K.copy()
    K[0, 1] = 0.7                      # skew
    K[2, 0], K[2, 1] = 1e-5, -2e-5     # a projective row: (K lpos)_2 != lpos_2, and K^-1's third row is full
    return K, np.linalg.inv(K)


def skewed_scene(sc):
    """A copy of the scene seen through skewed(K)."""
    K, Kinv = skewed(sc["K"])
    return dict(sc, K=K, Kinv=Kinv)


def start_volumes(sc, dtype=np.float64):
    T = np.full(sc["shape"], sc["tdist"] / sc["scale"], dtype=dtype)
    return T, np.zeros(sc["shape"], dtype=dtype)


def restate(sc, knn, weight="unit", wmax=100.0, dtype=np.float64, depths=None, K=None, Kinv=None, T=None, Wt=None):
    if T is None:
        T, Wt = start_volumes(sc, dtype)
    return integrate_depth_dqb_np(T, Wt, sc["depths"] if depths is None else depths, sc["lws"], sc["K"] if K is None else K,
                                  sc["Kinv"] if Kinv is None else Kinv, sc["scale"], sc["center"], sc["tdist"], sc["node_pos"],
                                  sc["node_dq"], sc["node_w"], knn, sc["lw_dq"], wmax=wmax, weight=weight, tsdf_res=sc["tsdf_res"])
