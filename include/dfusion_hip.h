/* dfusion_hip.h -- C ABI of libdfusion_hip.so, the MI355X (gfx950) implementation of the
 * per-frame DynamicFusion hot path of nintendops/DynamicFusion_Body.
 *
 * The reference has no FFI: its own device plug-in is a Python subclass overriding one
 * numpy-in/numpy-out method (class FusionDM_GPU, core/fusion_dm.py:563-574,600).  This
 * library is what such an override binds through ctypes; every entry
 * point names the reference function whose arithmetic it reproduces.
 *
 * Conventions
 *  - All array pointers are DEVICE pointers (hipMalloc / torch.Tensor.data_ptr()) unless
 *    the parameter is a small fixed-size `const double[...]`, which is HOST memory read
 *    during the call (mask arithmetic is fp64, so small matrices travel as doubles).
 *  - Volumes are C-ordered [x][y][z], z fastest (np.nditer order, core/fusion_dm.py:186;
 *    the OpenCL kernel's idx = x*RES_Z*RES_Y + y*RES_Z + z, :637).  A volume buffer holds
 *    the axis-0 planes [x0, x1) of a res[0] x res[1] x res[2] grid (slab partition across
 *    GPUs); voxel indices used in the arithmetic are always GLOBAL.
 *  - a volume's `dtype` / `depth_dtype`: DFH_F32 or DFH_F64. fp32 volumes are the product
 *    layout (16 B/voxel read-modify-write); fp64 volumes reproduce the reference's float64
 *    arrays bit for bit and exist for parity checking.
 *  - Calls are asynchronous on `stream` (a hipStream_t; NULL = default stream); dfh_radius_sample, which drives its rounds
 *    from the host, is the exception and says so.
 *  - Return value: 0 on success, <0 on error (DFH_E_*); dfh_last_error() describes the
 *    last failure on the calling thread.  Nothing throws across the ABI.
 */
#ifndef DFUSION_HIP_H
#define DFUSION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFH_ABI_VERSION 8

#define DFH_F32 0
#define DFH_F64 1

#define DFH_OK 0
#define DFH_E_BADARG (-1)
#define DFH_E_HIP (-2)
#define DFH_E_UNSUPPORTED (-3)
#define DFH_E_TIMEOUT (-4)
#define DFH_E_INTERNAL (-5)

/* ABI version of the loaded library (== DFH_ABI_VERSION of the header it was built from). */
int dfh_version(void);

/* Message for the last non-zero return on this thread ("" if none). */
const char *dfh_last_error(void);

/* Blocks until `stream` has drained (hipStreamSynchronize). */
int dfh_stream_synchronize(void *stream);

/* Development switches of the library (A/B experiments, tests that force a fall-back path).  They are NOT read from the
 * environment on the call paths: the table is filled once, at the first call into the library, from the single environment
 * variable DFH_OPTIONS="name=value,name=value" and is changed afterwards only through dfh_set_option().  Names are listed in
 * tools/README.md (e.g. "k1_no_bricks", "pcg_multilaunch", "pcg_spin_limit"); a value of -1 means "unset / library default".
 * dfh_set_option returns DFH_E_BADARG for an unknown name; dfh_get_option returns the current value (LONG_MIN if unknown).
 * No reference counterpart (the reference has no tuning switches). */
int dfh_set_option(const char *name, long value);
long dfh_get_option(const char *name);

/* ---- what the TSDF entry points (K1-K3) share, as structs in HOST memory read during the call.
 * dfh_slab: the axis-0 planes [x0, x1) of a res grid (> 0 each), 0 <= x0 <= x1 <= res[0], at most 65535 planes; voxel indices stay
 *   GLOBAL.  x0 == x1: nothing to do (DFH_OK before any launch, size queries give 0).  Anything else: DFH_E_BADARG (size queries 0).
 * dfh_volume: the T / w pair holding a slab's planes, both of `dtype`.  dfh_live: the WHOLE live volume. */
typedef struct dfh_slab { int res[3]; int x0, x1; } dfh_slab;
typedef struct dfh_volume { void *tsdf, *tsdf_w; int dtype; dfh_slab slab; } dfh_volume;
typedef struct dfh_live { const void *data; int dtype; int res[3]; } dfh_live;
typedef struct dfh_depth_views {     /* n_views depth maps of one size through one camera */
    int n_views;                     /* 0..16 */
    const void *const *depth;        /* HOST array of n_views device pointers: H x W row-major, negative depths, 0 = no measurement */
    int depth_dtype, H, W;           /* H, W >= 2 */
    double K[9], Kinv[9];            /* 3x3 row-major */
    const double *lw;                /* HOST, n_views x 12: a 3x4 row-major extrinsic per view */
    double scale, center[3];
    int tsdf_res;                    /* the ctor's tsdf_res (core/fusion_dm.py:60,:183) */
} dfh_depth_views;
/* the graph's nodes, device fp64: pos n_nodes x 3, dq n_nodes x 8, w n_nodes (the nodes' 4th tuple entry, 2*radius, core/fusion.py:116) */
typedef struct dfh_nodes { const double *pos, *dq, *w; int n_nodes, knn; /* 1 <= knn <= 8, knn <= n_nodes */ } dfh_nodes;

/* A1  FusionDM.fuseDepths(dm, lw, tsdf, tsdf_w, scale, center, wmax)  core/fusion_dm.py:180-217
 * (CPU-path semantics; the OpenCL variant :600-737 is NOT what is reproduced).
 * For every voxel i=(x,y,z), x in [x0,x1), and every view in turn:
 *   pos  = scale*(i - tsdf_res/2) + center                       (:183,:191)
 *   lpos = lw*[pos,1];  (u,v) = (K*lpos)_{0,1}/(K*lpos)_2, skipped if (K*lpos)_2 == 0   (:193-194)
 *   visible iff 0<=u<W-1 and 0<=v<H-1                            (:195)
 *   z = -depth[rint(v)][rint(u)] (round-half-even), valid iff z>0   (:196-197)
 *   sd = (Kinv*(z*[u,v,1]))_2 - lpos_2;  update iff sd > -tdist   (:198-203)
 *   T <- (scale*T*w + min(tdist,sd)) / (scale*(1+w));  w <- min(1+w, wmax)   (:209-210)
 * One view (n_views == 1).  workspace (may be NULL): device scratch of dfh_integrate_workspace_bytes(1, H, W, slab) bytes.  With it, float32
 * volumes are swept in 4 x 4 x 16 voxel bricks after a classification pass (same call, same stream) that marks the bricks
 * whose eight projected corners prove that the view updates none of their voxels -- outside the image, or behind the
 * surface by more than tdist according to a max-depth pyramid of the depth map -- and the sweep skips those: same result,
 * bit for bit, about half the projection work for a typical view.  Without it every voxel is projected.
 * Several views (n_views <= 16) go in ONE sweep of the volume: what the reference's loops over fuseDepths do
 * (core/fusion_dm.py:152-154 initial fusion, :166-170 compute_live_tsdf), with every voxel's T and w read once, updated
 * view by view in registers -- the float32 operations of consecutive one-view calls, so the same bits -- and written once.
 * workspace: device scratch; dfh_integrate_workspace_bytes(n_views, H, W, slab) bytes enable the brick
 * sweep with the per-(brick, view) classification described above (a brick runs only the views that may update it, a brick
 * no view updates is never loaded), dfh_integrate_multi_workspace_bytes(n_views)
 * bytes (the views' folded projection parameters only) the plain sweep; without a workspace, for float64 volumes and for
 * depth maps beyond 2048 pixels a side the call runs one sweep per view.
 * fresh_value != NULL, a live volume from scratch: the volumes are first set to (*fresh_value, 0) -- the reference's
 * np.zeros(...) + tdist and np.zeros(...) in front of its fuseDepths loops, core/fusion_dm.py:100-101,152-153 -- and the views are
 * then fused: the result is that of the two fills followed by the call without fresh_value, bit for bit (*fresh_value is rounded to
 * the volume's type).  With the column sweep the fill is part of the sweep: nothing is read and every voxel of the slab is written
 * once (a 256^3 live volume of three views: fills 38 + sweep 89 -> sweep 84 us); otherwise the slab is filled by a launch of its own first.
 * n_views == 0 only fills; without fresh_value it does nothing. */
size_t dfh_integrate_workspace_bytes(int n_views, int H, int W, const dfh_slab *slab);
size_t dfh_integrate_multi_workspace_bytes(int n_views);
int dfh_integrate_depth(const dfh_volume *vol, const dfh_depth_views *views, double tdist, double wmax,
                        const double *fresh_value /* NULL: keep the volumes */, void *workspace, size_t workspace_bytes, void *stream);

/* Which sweep a one-view dfh_integrate_depth takes for float32 volumes of this slab and depth-map size (no launch): one of
 * DFH_K1_PATH_*, the CLASS of bytes the sweep moves (several kernels may share one).  All of them produce the same volumes bit for
 * bit; they differ in the bytes they move (measurement code counts those of the path taken).  have_workspace: a workspace of dfh_integrate_workspace_bytes(1, ...) bytes will be passed.
 * No reference counterpart. */
#define DFH_K1_PATH_EXACT 0          /* every voxel through the reference's fp64 chain (fp64 volumes, oversized depth maps) */
#define DFH_K1_PATH_ROWS 1           /* T, w loaded and stored for updated 16-byte packs only (the row sweep; the gather-first column walk) */
#define DFH_K1_PATH_COLUMNS 2        /* T, w of every pack loaded, updated packs stored (the column walk over every 4 x 2 x 32 brick) */
#define DFH_K1_PATH_COLUMNS_CULLED 3 /* T, w of every pack of the bricks a depth pyramid + brick classification keep loaded, updated packs stored */
int dfh_integrate_depth_path(int vol_dtype, const dfh_slab *slab, int H, int W, int have_workspace);

/* A2 (optional)  the arithmetic of the reference's OpenCL kernel `fuse_depth`  core/fusion_dm.py:630-674 -- NOT that of the CPU
 * path above: index -> pixel through one float32 3x4 map proj = K lw IND (:640-646,:695), bilinear depth (:605-622), pixels without
 * or with near depth (pz <= tdist) carve free space (dz = -tdist, :652-653), dz = voxel depth - measured depth (:655-658), update
 * iff dz < tdist: w' = min(1 + w, wmax), T <- ((w' - 1) T + max(-tdist, dz)) / w', w <- w' (:667-672).  All float32, in the kernel
 * text's operation order, no contraction.  vol: float32 planes [x0,x1) (any other dtype: DFH_E_BADARG), updated in place (the reference's host code
 * copies its inputs first, :690-691); depth float32 H x W; tdist / wmax as the float literals the reference bakes in ("%ff" of
 * the Python values, :682-687).  A pixel coordinate that is NaN (w == 0) is skipped (undefined in the reference). */
int dfh_integrate_depth_ocl(const dfh_volume *vol, const float *depth, int H, int W,
                            const float proj[12], const float kinv_row2[3], float tdist, float wmax, void *stream);

/* A3  FusionDM.updateTSDF(curr_tsdf, wmax)                     core/fusion_dm.py:300-316
 * For every canonical voxel i, x in [x0,x1):
 *   q = dqb_warp(lw_dq, float32(i))          (core/util.py:68-72; lw_dq = `_lw`, 8 doubles, voxel-index
 *                                             space, may be non-unit after solve, fusion_dm.py:282)
 *   s = interpolate_tsdf(q, live)            (core/util.py:102-137: None outside [0,R-1]^3, ceil() upper
 *                                             corner, y/z fractions swapped -- reproduced)
 *   update iff s is not None and s > -tdist: T <- (T*w + min(tdist,s))/(1+w); w <- min(1+w, wmax)
 * live: the full live volume (every rank holds all of it: the warp gathers across slab boundaries). */
int dfh_fuse_volume_rigid(const dfh_volume *vol, const dfh_live *live, const double lw_dq[8], double tdist, double wmax, void *stream);

/* A4-A6  Fusion.updateTSDF(curr_tsdf, wmax)                    core/fusion.py:153-198
 * For every canonical voxel i, x in [x0,x1):
 *   loc = the knn nearest nodes of float32(i), nearest first       (KDTree.query(pos,k=knn+1)[1][:-1], :175-176)
 *   b   = sum_j exp(-(|i - v_j| / (2*w_j))^2) * dq_j ; b^ = b/|b|_8 (identity if |b|_8 == 0)   (dq_blend, :527-551)
 *   q   = dqb_warp(lw_dq, float32(dqb_warp(b^, i)))                (warp, :502-520; util.py:69)
 *   s   = interpolate_tsdf(q, live); update iff s is not None and s > -tdist              (:178-179)
 *   wi  = sum_j |v_j - i| / knn ; wt = w, or wi if w == 0                                 (:180-187)
 *   T <- (T*wt + min(tdist,s)*wi)/(wi + wt) ; w <- min(wi + wt, wmax)                      (:189-190)
 * nodes: dfh_nodes above.  workspace: device scratch of dfh_dqb_workspace_bytes() bytes
 * holding per-brick candidate node lists; they depend only on (node_pos, knn, grid, slab) and are rebuilt
 * when rebuild_candidates != 0.  A workspace of dfh_dqb_workspace_bytes_cached() bytes (16-byte aligned; the
 * plain size when n_nodes > 65536) additionally keeps per voxel the knn node indices (level 1: 2*knn bytes) and
 * the blend weights exp(..) and wi (level 2: + 8*(knn+1) bytes): the call with rebuild_candidates != 0 stores
 * them, later calls skip the node search and the sqrt/divide/exp chain -- same results, bit for bit, since
 * these values depend on (node_pos, node_w, knn, grid, slab) and not on node_dq.  The level in use is
 * inferred from workspace_bytes.
 * float32 volumes, knn = 4, level-2 workspace, lw_dq the identity, steady state (round 4): voxels that provably sample only
 * live voxels holding exactly tdist -- a per-brick bound on |warp(i) - i| from the brick's candidate nodes' DQs, a per-cell
 * "all 64 live voxels == tdist" mask -- skip the warp: s = tdist whatever the position; same bits (dfh_dqb_skip_layout;
 * option k3_skip = 0 switches it off). */
size_t dfh_dqb_workspace_bytes(const dfh_slab *slab);
size_t dfh_dqb_workspace_bytes_cached(const dfh_slab *slab, int knn, int n_nodes, int level);
int dfh_fuse_volume_dqb(const dfh_volume *vol, const dfh_live *live, const dfh_nodes *nodes, const double lw_dq[8], double tdist,
                        double wmax, void *workspace, size_t workspace_bytes, int rebuild_candidates, void *stream);

/* K1w  depth maps -> canonical volume through the warp field: DynamicFusion's surface fusion.  No reference counterpart as one
 * function: it composes Fusion.warp (core/fusion.py:502-551, as A4-A6 evaluate it) with FusionDM.fuseDepths' projection
 * (core/fusion_dm.py:191-203, as A1 evaluates it), so that the canonical update needs neither a live volume nor a second
 * trilinear resampling.  Everything is fp64 without contraction, for both volume dtypes.
 * For every canonical voxel i=(x,y,z), x in [x0,x1):
 *   loc, the Gaussian weights, b^, wi = sum_j |v_j - i| / knn and
 *   q   = dqb_warp(lw_dq, float32(dqb_warp(b^, i)))                are those of A4-A6: same neighbour order and tie rule, same
 *                                                                  8-norm, the identity blend when |b|_8 == 0
 * and then for every view 0 .. n_views-1 in turn, A1's chain with the index i replaced by q:
 *   pos  = scale*(q - tsdf_res/2) + center
 *   lpos = lw*[pos,1];  (u,v) = (K*lpos)_{0,1}/(K*lpos)_2, skipped if (K*lpos)_2 == 0
 *   visible iff 0<=u<W-1 and 0<=v<H-1
 *   z = -depth[rint(v)][rint(u)] (round-half-even), valid iff z>0; a z*u or z*v that is not finite updates nothing
 *   sd = (Kinv*(z*[u,v,1]))_2 - lpos_2;  update iff sd > -tdist    (tdist in the depth maps' units, as for A1)
 *   weight_mode DFH_WARPED_W_UNIT (A1's rule):
 *     T <- (scale*T*w + min(tdist,sd)) / (scale*(1+w));  w <- min(1+w, wmax)
 *   weight_mode DFH_WARPED_W_NODE_DISTANCE (A4-A6's rule, core/fusion.py:180-190: canonical weights keep their meaning when a
 *   frame loop switches between this call and dfh_fuse_volume_dqb):
 *     wt = w, or wi if w == 0;  T <- (T*wt + (min(tdist,sd)/scale)*wi) / (wi + wt);  w <- min(wi + wt, wmax)
 *   T and w are rounded to the volume's dtype after every view: n_views views in one call equal n_views one-view calls bit for
 *   bit, while the voxel is read once and written once (and only if a view updated it).
 * With every node DQ and lw_dq the identity (or every node DQ zero) q == i exactly, and DFH_WARPED_W_UNIT on float64 volumes
 * gives dfh_integrate_depth's bits.
 * workspace: the buffer of dfh_fuse_volume_dqb (dfh_dqb_workspace_bytes[_cached]); one buffer can serve both entry points.
 * rebuild_candidates != 0 builds the per-brick candidate lists, searches, and stores every voxel's knn node indices when the
 * buffer has room for them (level >= 1); rebuild_candidates == 0 loads stored indices when the buffer has them (clamped to
 * n_nodes - 1: a stale buffer cannot fault) and otherwise searches the existing lists.  The blend weights are always
 * recomputed from the node positions; the weight region of a level-2 buffer is never read or written.  Storing indices drops
 * the library's note of which dfh_fuse_volume_dqb path last wrote that region, so a later dfh_fuse_volume_dqb call without a
 * rebuild recomputes its weights from the stored indices (same bits) until its own next rebuild.
 * DFH_E_BADARG before any HIP call for: a bad volume or slab; null views, nodes, lw_dq or node arrays; n_views outside 0..16; a
 * null depth pointer; H or W < 2; a depth dtype other than DFH_F32 / DFH_F64; scale == 0; knn outside 1..8; n_nodes < knn; an
 * unknown weight_mode; a workspace smaller than dfh_dqb_workspace_bytes().  An empty slab or n_views == 0: DFH_OK, no launch. */
#define DFH_WARPED_W_UNIT 0
#define DFH_WARPED_W_NODE_DISTANCE 1
int dfh_integrate_depth_dqb(const dfh_volume *vol, const dfh_depth_views *views, const dfh_nodes *nodes,
                            const double lw_dq[8], double tdist, double wmax, int weight_mode,
                            void *workspace, size_t workspace_bytes, int rebuild_candidates, void *stream);

/* ---- warp-field solve ------------------------------------------------------------------------------
 * All arrays device fp64 unless noted; point / normal / node arrays are row-major (n x 3, n x 8).
 *
 * A9   FusionDM.computef_lw(x)                                   core/fusion_dm.py:285-297
 *   out[i] = dqb_warp_normal(x, normals[i]) . (dqb_warp(x, verts[i]) - corr[i])
 *   (verts/normals already restricted to `_corridx`; row i pairs with corr[i]). */
int dfh_residual_rigid(const double *verts, const double *normals, const double *corr, int n, const double x[8],
                       double *out, void *stream);

/* Rigid Gauss-Newton normal equations of 0.5*|computef_lw(x)|^2 for the left twist on x:
 * out44[0..35] = J^T J (6x6 row-major), out44[36..41] = J^T r, out44[42] = 0.5|r|^2, out44[43] = rows
 * used.  valid (uint8 per row) may be NULL. */
int dfh_gn_build_rigid(const double *verts, const double *normals, const double *corr, const unsigned char *valid, int n,
                       const double x[8], double *out44, void *stream);

/* A10  data rows of Fusion.computef(x, tdw, trw, rw) / Fusion.computef_lw   core/fusion.py:444-473
 *   (x', n') = warp(verts[s], node_dq[nbr[s]], nbr[s], normals[s], m_lw=lw_dq)   (:502-520)
 *   out[s] = n' . (x' - corr[s]);  nbr: n_verts x knn int32 (`_neighbor_look_up`, :121-123). */
int dfh_residual_data(const double *verts, const double *normals, const double *corr, const int *nbr, int n_verts,
                      int knn, const double *node_dq, const double *node_pos, const double *node_w, int n_nodes,
                      const double lw_dq[8], double *out, void *stream);

/* A10  regularisation rows of Fusion.computef                      core/fusion.py:475-484
 *   node_nbr[i][j] = _neighbor_look_up[_nodes[i][0]][j]  (n_nodes x knn int32)
 *   out[(i*knn + j)*3 + c] = rw * max(w_i, w_j) * (dqb_warp(dq_i, v_j) - dqb_warp(dq_j, v_j))[c]. */
int dfh_residual_reg(const int *node_nbr, int n_nodes, int knn, const double *node_dq, const double *node_pos,
                     const double *node_w, double rw, double *out, void *stream);

/* A5 for a batch: Fusion.warp(v, dqs[nbr], nbr, normal=n, m_lw=lw_dq) (core/fusion.py:502-520) for every
 * vertex; nbr == NULL applies only lw_dq (dqb_warp(_lw, v), dqb_warp_normal(_lw, n), fusion_dm.py:230-231).
 * normals / out_nrm may both be NULL. */
int dfh_warp_points(const double *verts, const double *normals, const int *nbr, int n_verts, int knn, const double *node_dq,
                    const double *node_pos, const double *node_w, int n_nodes, const double lw_dq[8], double *out_pos,
                    double *out_nrm, void *stream);

/* The selection loop of setupCorrespondences (core/fusion_dm.py:229-244; core/fusion.py:258-276, 'clpts'):
 * for every warped vertex the knn nearest live vertices (nearest first), best = the first with the smallest
 * cost |wn . (vp - p)| below the initial best_cost 1 (else the nearest), keep = best_cost <= tolerance.
 * corr_out n x 3, cost_out n (may be NULL), keep_out n uint8.
 * A warped vertex whose position is not finite (NaN or +-inf in any coordinate; in general: fewer than knn live vertices at a
 * finite squared distance) has no neighbours: corr_out = (0, 0, 0), cost_out = +inf, keep_out = 0.  A NaN normal at a finite
 * position is the reference's case "no cost below 1": best = the nearest, cost = 1. */
int dfh_closest_correspondences(const double *warped_pos, const double *warped_nrm, int n_verts, const double *live_verts,
                                int n_live, int knn, double tolerance, double *corr_out, double *cost_out,
                                unsigned char *keep_out, void *stream);

/* k nearest nodes (nearest first; KDTree.query order, core/fusion.py:121-123) and the Gaussian DQB
 * weights exp(-(|p - v_j| / (2 w_j))^2) (:537) of arbitrary sample points.  Both are static while the
 * graph is unchanged.  nbr_out: n_samples x knn int32; weights_out: n_samples x knn.
 * A sample whose position is not finite (in general: fewer than knn nodes at a finite squared distance) has no neighbours:
 * nbr_out = 0 .. knn-1 and every weight 0 (valid indices, a vanishing blend); the finite samples around it are unaffected.
 * dfh_sample_knn_bricks does the same. */
int dfh_sample_knn(const double *sample_pos, int n_samples, const double *node_pos, const double *node_w, int n_nodes,
                   int knn, int *nbr_out, double *weights_out, void *stream);
/* Where the constant-live skip of dfh_fuse_volume_dqb (float32 volumes, knn = 4, stored neighbourhoods, m_lw = identity; round 4)
 * keeps its per-call tables inside a level-2 workspace, as byte offsets from the workspace's start: out[0] live-cell mask U,
 * [1] slab-cell mask S, [2] per-brick reach (uint8: 1 / 2 cells, 255 = no bound), [3] per-brick displacement bound (float32,
 * voxels; -1 = not computed), [1] is one byte per brick (1 = constant-live stream, 0 = warp kernel), [4], [5] unused; [6..8] live cells
 * along x, y and 64-bit words per cell row, [9..10] slab cell rows; [11] 1 when these sizes admit the skip at all; [12] per brick
 * the 16 node ids (uint16, ascending, 0xffff = none, first = 0xfffe: too many) its voxels blend.  For tests and measurement code:
 * the proof obligation "no voxel moves further than its brick's bound" is checked against [3] (tests/test_gpu_fuse_volume.py).
 * No reference counterpart. */
int dfh_dqb_skip_layout(const dfh_slab *slab, const int live_res[3], int knn, int n_nodes, size_t out[13]);
/* The same through the per-brick candidate lists of a dfh_fuse_volume_dqb workspace (built for the same node_pos, knn,
 * grid and slab by dfh_dqb_build_candidates or by a dfh_fuse_volume_dqb call with rebuild_candidates != 0): a point
 * scans the list of the brick of its nearest voxel centre (the lists carry the head-room that makes this exact for
 * off-lattice points); points outside the slab's lattice and bricks whose list overflowed scan every node.
 * Same output as dfh_sample_knn, bit for bit.  An empty slab (x0 == x1) has no lists: both calls return DFH_OK and write nothing
 * (dfh_sample_knn is the call for such points). */
int dfh_dqb_build_candidates(const dfh_slab *slab, const double *node_pos, int n_nodes, int knn,
                             void *workspace, size_t workspace_bytes, void *stream);
int dfh_sample_knn_bricks(const double *sample_pos, int n_samples, const double *node_pos, const double *node_w,
                          int n_nodes, int knn, const dfh_slab *slab, const void *workspace,
                          size_t workspace_bytes, int *nbr_out, double *weights_out, void *stream);

/* ---- deformation-graph maintenance: the device side of Fusion.update_graph / construct_graph ---------------------
 * (core/fusion.py:101-123, 201-239; the greedy radius subsampling of the unsupported vertices, core/util.py:27-47, is
 * dfh_radius_sample below).
 * dfh_nearest_points: idx_out[q] = nearest cloud point of query q (KDTree(cloud).query(q), :209-212 -- a node's anchor
 *   vertex; ties go to the lower index), d2_out (may be NULL) its squared distance.  A query that is not finite (no cloud
 *   point at a finite squared distance): idx_out = -1, d2_out = +inf.
 * dfh_graph_unsupported: flag_out[v] = 1 iff min over the vertex's knn nodes nbr[v][.] of |node - v| / node_w >= 1
 *   (the "unsupported surface point" test, :215-219).
 * dfh_dq_blend_points: dq_out[p] = Fusion.dq_blend(points[p]) over the nodes nbr[p][.] (:527-551; the DQ a newly
 *   inserted node starts from, :222), 8 doubles per point. */
int dfh_nearest_points(const double *query, int n_query, const double *cloud, int n_cloud, int *idx_out, double *d2_out, void *stream);
int dfh_graph_unsupported(const double *verts, int n_verts, const int *nbr, int knn, const double *node_pos, const double *node_w,
                          int n_nodes, unsigned char *flag_out, void *stream);
int dfh_dq_blend_points(const double *points, int n_points, const int *nbr, int knn, const double *node_dq, const double *node_pos,
                        const double *node_w, int n_nodes, double *dq_out, void *stream);

/* Greedy radius subsampling (core/util.py:27-47: take the first remaining candidate, drop every candidate closer than `radius`
 * to it, repeat) of n_points fp64 points p_0 .. p_{n-1} (n_points x 3).  The selected set A is
 *      i in A  <=>  no j < i with j in A and dist(p_i, p_j) < radius,
 * the lexicographically first maximal independent set of the "closer than radius" graph, built in parallel rounds over a uniform
 * cell table; it is the host loop's result index for index.  dist is computed operation by operation in fp64 with no
 * contraction: d = p_i - p_j per component, s = (d0 d0 + d1 d1) + d2 d2, dist = sqrt(s) correctly rounded, and the comparison is
 * strict: a point at distance exactly `radius` from a selected point is kept, duplicates of a selected point are dropped.
 * idx_out (device, `capacity` int32): the min(count, capacity) lowest selected indices in ascending order, which is the order the
 * host loop returns them in.  count_out, rounds_out: HOST pointers (rounds_out may be NULL): |A|, and the number of rounds run.
 * workspace: dfh_radius_sample_workspace_bytes(n_points) bytes of device memory, 8-byte aligned; the size is a function of
 * n_points only (the cell table is capped and the cells grow to fit the bounding box: a far outlier costs rounds, never memory).
 * UNLIKE the other entry points this call does not only enqueue: it queues its rounds on `stream` a few at a time, synchronises
 * `stream` in between to read how many points are still undecided, and has written count_out when it returns.  It cannot be
 * captured into a graph.  At most n_points rounds run (every round decides at least the lowest undecided index); a round that
 * decides nothing returns DFH_E_INTERNAL.
 * n_points == 0: DFH_OK with count 0 before any launch.  DFH_E_BADARG before any HIP call: n_points < 0 or >= 2^31; radius not
 * finite or <= 0; capacity < 0; null count_out; with n_points > 0 a null points, idx_out or workspace, or a workspace that is
 * too small.  Coordinates that are not finite are the caller's error (the host loop never terminates on them); the call still
 * terminates and touches no memory outside its arguments. */
size_t dfh_radius_sample_workspace_bytes(long n_points);
int dfh_radius_sample(const double *points, long n_points, double radius, int *idx_out, long capacity, long *count_out,
                      int *rounds_out, void *workspace, size_t workspace_bytes, void *stream);

/* out[i] = in[order[i]] for the four per-sample arrays at once (samples are sorted by node tuple before the build:
 * few runs per tile of dfh_gn_tile_samples() samples).  order: n_samples int64 indices, a permutation. */
int dfh_permute_samples(const long *order, int n_samples, int knn, const double *pos, const double *nrm, const int *nbr,
                        const double *weights, double *pos_out, double *nrm_out, int *nbr_out, double *weights_out, void *stream);

/* The Gauss-Newton problem the solver owns: samples, nodes, term settings, the block system and the plans of its build.
 * Gauss-Newton normal equations of 0.5*|computef|^2 in 6-DoF left twists (dq_a <- exp(xi_a) (x) dq_a): vals <- J^T J,
 * rhs <- J^T r, cost_count[0] <- 0.5 |r|^2 (the Huber objective with huber_delta > 0), cost_count[1] <- valid samples. */
typedef struct dfh_gn_problem {
    /* samples, sorted by node tuple for the planned build: positions and normals (n_samples x 3), their knn nearest nodes
     * (n_samples x knn int32) and static blend weights (dfh_sample_knn); corr (n_samples x 3, index space) / valid (uint8):
     * inputs of a build without a frame, outputs of an association.  1 <= knn <= 8. */
    const double *sample_pos, *sample_nrm;
    const int *nbr;
    const double *weights;
    double *corr;
    unsigned char *valid;
    int n_samples, knn;
    /* nodes: node_dq (n_nodes x 8, updated by dfh_gn_solve), positions (x 3), weights (the 4th tuple entry, 2*radius);
     * node_nbr (n_nodes x knn int32; NULL: no regulariser rows) = _neighbor_look_up[_nodes[i][0]][j]. */
    double *node_dq;
    const double *node_pos, *node_w;
    const int *node_nbr;
    int n_nodes;
    /* lw_dq: the rigid part `_lw`; rw: the regulariser weight (0: no regulariser rows); huber_delta > 0:
     * every data row and its residual are scaled by sqrt(min(1, huber_delta / |r|)), the IRLS form of the Huber loss of the
     * reference's solver (least_squares(loss='huber'), core/fusion.py:389); 0 = plain least squares. */
    double lw_dq[8];
    double rw, huber_delta;
    /* the block system: vals (n_blocks x 36) in block-sparse rows row_ptr (n_nodes + 1) / col (sorted), rhs (6 n_nodes),
     * cost_count (2).  The pattern must contain every node pair of every sample tuple and every (i, j) of node_nbr (both
     * orders) plus the diagonal; missing blocks are silently dropped.  blk_upper (n_upper pairs of ints; NULL / 0: none): for
     * every block with column >= row {its index, its mirror block's (column, row), -1 on the diagonal}; with it the gather walks
     * only those blocks and stores every sum twice, the second time transposed: the same bits, half the walks. */
    const int *row_ptr, *col;
    int n_blocks;
    double *vals, *rhs, *cost_count;
    const int *blk_upper;
    int n_upper;
    /* the data plan (dfh_gn_plan_build; static while the samples are): a "row" = a maximal run of equal tuples inside one
     * tile of dfh_gn_tile_samples() samples.  run_id[s] = row of sample s (n_rows rows); partial: scratch of
     * n_rows x dfh_gn_partial_doubles(knn) + 2 x ceil(n_samples / dfh_gn_tile_samples()) + n_rows doubles; blk_ptr (n_blocks + 1)
     * / blk_ent: per block the entries row * knn^2 + sa * knn + sb; node_ptr (n_nodes + 1) / node_ent: per node the entries
     * row * knn + slot.  The tile pass stores each row's Gram matrix, J^T r, cost and count, a gather adds them per block: no
     * floating-point atomics, the same bits every run.  blk_ptr == NULL: the data rows go to the blocks through atomics. */
    const int *run_id;
    int n_rows;
    double *partial;
    const int *blk_ptr, *blk_ent, *node_ptr, *node_ent;
    /* the regulariser's plan: partial_reg (n_nodes * knn rows of dfh_gn_partial_doubles(2) doubles) and its lists, a pair
     * (i, node_nbr[i*knn+slot]) being a 2-node row (entries row * 4 + sa * 2 + sb, row * 2 + slot).  partial_reg == NULL (or
     * an atomic build) keeps the regulariser on atomics. */
    double *partial_reg;
    const int *rblk_ptr, *rblk_ent, *rnode_ptr, *rnode_ent;
} dfh_gn_problem;

/* The live frame the data term is associated against (projective association, not in the reference, which matches
 * marching-cubes vertices through a KD-tree, core/fusion.py:255-276): each sample is warped with the current field
 * (Fusion.warp), mapped index -> world (pos = scale*(i - half) + center, fusion_dm.py:191) -> camera (the view's lw_cam,
 * :193) -> pixel (:194-195); the nearest depth pixel z = -depth[rint(v)][rint(u)] (:196) is back-projected, K^-1 (z [u,v,1])
 * (:198-200), and mapped back to index space.  A view gives no correspondence outside the image, without depth, or farther
 * than max_dist voxels from the warped sample (max_dist <= 0: no gate).  With several views a sample keeps the view in which
 * it lies closest to the observed surface (ties go to the lower view index): still ONE data row per sample.  Oracle:
 * gn_np.associate_depth_views. */
typedef struct dfh_gn_frame {
    const void *views;       /* a dfh_gn_pack_views table (device) of n_views (1..DFH_GN_MAX_VIEWS) maps of depth_dtype */
    int n_views, depth_dtype;
    int H, W;                /* the maps' size, >= 2 each */
    double K[9], Kinv[9];    /* intrinsics and their inverse, 3x3 row-major */
    double scale;            /* index -> world: scale * (i - half) + center; scale != 0 */
    double center[3];
    double half;
    double max_dist;         /* the distance gate in voxels (<= 0: none) */
} dfh_gn_frame;

/* One call's solve schedule (dfh_gn_solve). */
typedef struct dfh_gn_solve_params {
    int pcg_iters;                        /* the PCG of dfh_pcg_solve_update (>= 1) on the system of each iteration's build */
    double lm_abs, lm_rel;
    double *x_out;                        /* 6 n_nodes: the last iteration's step */
    void *pcg_workspace;                  /* dfh_pcg_workspace_bytes(n_nodes, pcg_iters) bytes */
    size_t pcg_workspace_bytes;
    double step;                          /* node_dq <- exp(step * x) node_dq */
    int n_iters;                          /* node iterations, 0..1000 */
    int n_global;                         /* rigid-mode steps in front of them, 0..100 (dfh_gn_global_step(global_lm)) */
    double global_lm;
    double *global_xi_out;                /* may be NULL */
    void *global_scratch;                 /* dfh_gn_global_step_bytes(), zeroed once by the caller */
    size_t global_scratch_bytes;
} dfh_gn_solve_params;

/* The views' table of a frame, written into `out`, a device buffer of dfh_gn_views_bytes(n_views, depth_dtype, H, W) bytes,
 * once per frame: extrinsics, their inverses, depth pointers.  depth[v]: host array of device pointers to H x W maps of
 * depth_dtype; lw_cam: 12 doubles per view (host).  For DFH_F32 maps the table also holds, per view, the 16 x 16-pixel cells'
 * {smallest, largest valid z = -depth}: with them the fused builds drop, per 128-sample tile, the views none of its samples can
 * be valid in (the tile's warped box projects outside the image, or onto pixels whose valid depths all lie further than
 * max_dist from the box's depth range; exact for rigid extrinsics and a pinhole K) -- the same corr / valid, the same bits
 * (option gn_no_view_cull = 1 keeps every view).  DFH_F64 maps get no cells. */
#define DFH_GN_MAX_VIEWS 16
size_t dfh_gn_views_bytes(int n_views, int depth_dtype, int H, int W);
int dfh_gn_pack_views(void *out, int n_views, const void *const *depth, int depth_dtype, int H, int W, const double *lw_cam,
                      void *stream);

/* corr / valid of the problem's samples against the frame (no system is touched). */
int dfh_gn_associate(const dfh_gn_problem *problem, const dfh_gn_frame *frame, void *stream);

/* The volume data term: corr / valid of the problem's samples against a live TSDF VOLUME (no system is touched; the contract of
 * dfh_gn_associate: reads the samples, nbr, weights, node_dq, lw_dq and knn, writes corr and valid; dfh_gn_build(problem, NULL)
 * then builds from them).  One trilinear cell per sample, whatever the number of views that were fused into the volume.  Not in
 * the reference, whose Fusion.setupCorrespondences(volume) runs marching cubes on the live volume and a KD-tree search
 * (core/fusion.py:255-276).  Everything is fp64, operation by operation in this order, no contraction:
 *  1. x' = (X0, X1, X2): the sample warped exactly as dfh_gn_associate warps it (the normalised static blend of its knn node DQs,
 *     then dqb_warp with the blend and with lw_dq, positions rounded to float32 where Fusion.warp rounds them).
 *  2. in grid: per axis a, 0 <= Xa and Xa < res[a] - 1, tested on the doubles (NaN and infinities fail); ia = floor(Xa),
 *     fa = Xa - ia.
 *  3. corners u[a][b][c] = (double)live[((i0+a)*res[1] + (i1+b))*res[2] + (i2+c)] * value_to_vox: the STANDARD trilinear cell, f0
 *     with axis 0, f1 with axis 1, f2 with axis 2 -- NOT interpolate_tsdf's sampler (core/util.py:102-137: ceil() corners, y / z
 *     fractions swapped), the reference's quirk that dfh_fuse_volume_rigid / _dqb reproduce for updateTSDF only.
 *  4. band: all eight corners satisfy fabs(u) < band (strict; a NaN corner fails).  A voxel a fresh dfh_integrate_depth sweep never
 *     updated holds exactly tdist: with band = tdist the cells behind the surface and in free space drop out without a weight volume.
 *  5. e[a][b] = u[a][b][0] + f2*(u[a][b][1] - u[a][b][0]);  h[a] = e[a][0] + f1*(e[a][1] - e[a][0]);  s = h[0] + f0*(h[1] - h[0]);
 *     g0 = h[1] - h[0];  dy[a] = e[a][1] - e[a][0], g1 = dy[0] + f0*(dy[1] - dy[0]);  dz[a][b] = u[a][b][1] - u[a][b][0],
 *     m[a] = dz[a][0] + f1*(dz[a][1] - dz[a][0]), g2 = m[0] + f0*(m[1] - m[0])     (s and its gradient g at x', in voxels).
 *  6. G = (g0*g0 + g1*g1) + g2*g2; usable iff G >= min_grad*min_grad and G > 0 (always: t below divides by it); with
 *     max_dist > 0 also s*s <= (max_dist*max_dist)*G, i.e. |c - x'| <= max_dist without a square root.
 *  7. t = s / G, corr = x' - t*g (one Newton step onto the zero level set of the interpolant), valid = 1.  If any test fails:
 *     valid = 0 and corr = (0, 0, 0) -- every row is written on every call.
 * DFH_E_BADARG (before any HIP call): null problem / term / node_dq / live.data, null sample_pos / nbr / weights / corr / valid
 * with n_samples > 0, knn outside 1..8, n_nodes < 1, n_samples < 0, a live dtype other than DFH_F32 / DFH_F64, a res < 2,
 * value_to_vox zero or not finite, band not > 0, min_grad negative or NaN, max_dist NaN.  n_samples == 0: DFH_OK, no launch. */
typedef struct dfh_gn_volume_term {
    dfh_live live;        /* the WHOLE live volume, z fastest, DFH_F32 or DFH_F64, every res >= 2 */
    double value_to_vox;  /* stored value * value_to_vox = distance in voxels; finite, != 0 */
    double band;          /* > 0, voxels: a cell is usable iff all 8 corners have |u| < band (strict) */
    double max_dist;      /* gate in voxels on |c - x'|; <= 0: none */
    double min_grad;      /* >= 0: usable iff |g|^2 >= min_grad^2 */
} dfh_gn_volume_term;
int dfh_gn_associate_volume(const dfh_gn_problem *problem, const dfh_gn_volume_term *term, void *stream);

/* The normal equations of the problem.  frame == NULL: corr / valid are inputs.  frame != NULL: the association is fused into
 * the data-row kernel -- every sample is warped once, associated as by dfh_gn_associate (corr / valid receive the same values,
 * bit for bit) and the valid ones go straight on to their Jacobian rows; it needs the data plan and DFH_F32 maps. */
int dfh_gn_build(const dfh_gn_problem *problem, const dfh_gn_frame *frame, void *stream);
/* dfh_gn_build with a frame, for volumes: the cell evaluation of dfh_gn_associate_volume (steps 1-7 above, the same operations)
 * runs inside the data-row kernel.  corr / valid and vals / rhs / cost_count are, bit for bit, those of dfh_gn_associate_volume
 * followed by dfh_gn_build(problem, NULL).  It needs the data plan (blk_ptr != NULL) and a DFH_F32 live volume (DFH_F64 volumes
 * keep the two calls, as DFH_F64 depth maps do).  DFH_E_BADARG (before any HIP call): what dfh_gn_build and
 * dfh_gn_associate_volume refuse, a problem without a plan, a DFH_F64 volume. */
int dfh_gn_build_volume(const dfh_gn_problem *problem, const dfh_gn_volume_term *term, void *stream);
size_t dfh_gn_partial_doubles(int knn);

/* Samples per tile of the planned build (a scratch row = a run of equal node tuples inside one tile; callers size tile_off,
 * the per-tile {cost, count} pairs behind the scratch rows and the torch restatement of the plan with it). */
int dfh_gn_tile_samples(void);

/* ---- per-frame bookkeeping of the planned build, on the device ---------------------------------------------------------
 * dfh_gn_sort_samples: the four per-sample arrays in the order of their node tuples (lexicographic, stable: equal tuples
 *   keep their input order), key_out[i] = the i-th sorted tuple as a knn-digit number in base n_nodes, order_out[i] =
 *   input index of the i-th sorted sample.
 * dfh_gn_plan_count:   rows = maximal runs of equal tuples inside tiles of dfh_gn_tile_samples() samples of the SORTED nbr; tile_off
 *   (ceil(n_samples / dfh_gn_tile_samples()) + 1 ints) <- first row of every tile, *n_rows_out (device) <- number of rows.
 *   (*n_rows_out, like *uncovered_out below and dfh_surface_count's *total_out, is written by ONE plain store of the sequence's
 *   last writer: it may be device memory or pinned host memory, which the host can then watch instead of queueing a copy.)
 * dfh_gn_plan_build:   run_id (n_samples), row_first (n_rows: first sample of every row) and the CSR lists of
 *   dfh_gn_problem -- blk_ptr (n_blocks + 1) / blk_ent (n_rows * knn^2), node_ptr (n_nodes + 1) / node_ent (n_rows * knn),
 *   every list in ascending entry order; *uncovered_out (device int) <- 1 if some node pair of some row is not a block
 *   of the pattern (row_ptr / col), its entries are left out.  n_rows is the value dfh_gn_plan_count produced. */
size_t dfh_gn_sort_workspace_bytes(int n_samples);
int dfh_gn_sort_samples(const double *pos, const double *nrm, const int *nbr, const double *weights, int n_samples, int knn,
                        int n_nodes, double *pos_out, double *nrm_out, int *nbr_out, double *weights_out, long *key_out,
                        int *order_out, void *workspace, size_t workspace_bytes, void *stream);
int dfh_gn_plan_count(const int *nbr, int n_samples, int knn, int *tile_off, int *n_rows_out, void *stream);
size_t dfh_gn_plan_workspace_bytes(int n_rows, int knn);
int dfh_gn_plan_build(const int *nbr, int n_samples, int knn, int n_nodes, const int *tile_off, int n_rows, const int *row_ptr,
                      const int *col, int n_blocks, int *run_id, int *row_first, int *blk_ptr, int *blk_ent, int *node_ptr,
                      int *node_ent, int *uncovered_out, void *workspace, size_t workspace_bytes, void *stream);

/* Block-Jacobi preconditioned CG on (A + lm_abs I + lm_rel diag(A)) x = -rhs, `iters` iterations, no
 * host synchronisation.  The damping is written into vals' diagonal (vals is consumed). */
size_t dfh_pcg_workspace_bytes(int n_nodes, int iters);
int dfh_pcg_solve(const int *row_ptr, const int *col, double *vals, const double *rhs, int n_nodes, int iters,
                  double lm_abs, double lm_rel, double *x_out, void *workspace, size_t workspace_bytes, void *stream);

/* dfh_pcg_solve followed by the twist update node_dq[a] <- exp(step * x_out[a]) (x) node_dq[a] (dfh_apply_twist's arithmetic), in
 * the same launch where the persistent kernel runs: one GN iteration's solve + update.  On BOTH paths the update is all or
 * nothing: it is applied only if every entry of x_out is finite; a NaN or an infinity anywhere in x_out (a non-finite rhs or
 * matrix, a timed-out barrier) leaves node_dq bit for bit as it was before the call. */
int dfh_pcg_solve_update(const int *row_ptr, const int *col, double *vals, const double *rhs, int n_nodes, int iters,
                         double lm_abs, double lm_rel, double *x_out, void *workspace, size_t workspace_bytes, double *node_dq,
                         double step, void *stream);

/* A single-GPU solve behind one call: params->n_global rigid-mode steps (a fused build + dfh_gn_global_step each), then
 * params->n_iters node iterations, each a fused build followed by dfh_pcg_solve_update on the system it produced -- the same
 * bits as the separate calls.  Knowing both halves, the library lets the clearing of the solve's workspace ride in the data-row
 * launch; the iterations are queued back to back (nothing between them depends on the host).  frame: DFH_F32 maps; the problem
 * needs its data plan.  Multi-GPU solves keep the separate calls (the all-reduce goes between build and solve).  Reference: the
 * body of least_squares' iteration for Fusion.computef, core/fusion.py:356-389. */
int dfh_gn_solve(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_solve_params *params, void *stream);
/* dfh_gn_solve with the volume data term: the same schedule (params->n_global x [dfh_gn_build_volume -> dfh_gn_global_step], then
 * params->n_iters x [dfh_gn_build_volume with the solve workspace's clearing riding in its data-row launch -> the PCG and twist
 * update of dfh_pcg_solve_update]), the same bits as the separate calls (also as dfh_gn_associate_volume -> dfh_gn_build(problem,
 * NULL) -> dfh_gn_global_step / dfh_pcg_solve_update).  term: a DFH_F32 live volume; the problem needs its data plan.  Refuses what
 * dfh_gn_build_volume and dfh_gn_solve refuse. */
int dfh_gn_solve_volume(const dfh_gn_problem *problem, const dfh_gn_volume_term *term, const dfh_gn_solve_params *params, void *stream);

/* The normal-compatibility gate of the depth data term (opt-in: the calls above know nothing of it).  dfh_gn_associate accepts a
 * view's correspondence when the sample projects inside the image, the pixel has depth and |c - x'| <= max_dist; on anything
 * thinner than max_dist, and under an orbit of cameras, that matches samples to the far side of what they sit on.  With a gate the
 * view's correspondence must also face the way the model surface does: the live normal of the pixel the depth came from
 * (dfh_depth_prep's maps: camera space, flipped to face the camera) against the sample's warped normal (the TSDF gradient, which
 * points into free space: the two agree on a visible surface, so "compatible" is a POSITIVE cosine).  KinectFusion and
 * DynamicFusion reject such pairs the same way; the reference (mesh-to-mesh correspondences, core/fusion.py:255-276) has no
 * counterpart.  Everything is fp64, operation by operation in this order, no contraction.  For a sample:
 *  1. n' = its normal warped exactly as the data row warps it, the same functions and the same bits:
 *     dqb_warp_normal(lw_dq, f32(dqb_warp_normal(b^, f32(n)))), b^ the normalised static blend of its knn node DQs.
 *  2. for view v and the pixel (ui, vi) = (rint(u), rint(v)) dfh_gn_associate takes the depth from:
 *     l = the three floats at ((v*H + vi)*W + ui)*3 of `normals`, widened to double;
 *     m_i = (R_i0*n'_x + R_i1*n'_y) + R_i2*n'_z, R the 3x3 part of that view's lw_cam;
 *     d = sgn*((m_0*l_0 + m_1*l_1) + m_2*l_2), sgn = +1 if scale > 0, else -1;
 *     mm = (m_0*m_0 + m_1*m_1) + m_2*m_2, ll = (l_0*l_0 + l_1*l_1) + l_2*l_2.
 *  3. the view's correspondence passes iff d > 0 and d*d >= (min_cos*min_cos)*(mm*ll): no square root, scale-free in l and n'.  A
 *     NaN anywhere fails, and so does a pixel without a normal (l = 0: d = 0).
 *  4. the test sits beside the distance gate, BEFORE the "smallest |c - x'|^2 wins, ties to the lower view" comparison: a rejected
 *     nearer view lets a farther compatible one win.  The gate only removes correspondences, so the fused builds' per-tile view
 *     cull stays exact.
 * Restated in tests/assoc_normals_np.py.  Each call below has its ungated twin's contract -- what it reads and writes, the bits
 * of everything the gate lets through, float32 / float64 maps and the plan where the twin needs them -- plus the gate, and
 * additionally reads sample_nrm where the twin did not (dfh_gn_associate_gated).  dfh_gn_build_gated: corr / valid / vals / rhs /
 * cost_count are, bit for bit, those of dfh_gn_associate_gated followed by dfh_gn_build(problem, NULL); dfh_gn_solve_gated: the
 * schedule of dfh_gn_solve with dfh_gn_build_gated as its build, the same bits as the separate calls.  DFH_E_BADARG (before any HIP
 * call): everything the twin refuses, a null gate, null normals, min_cos NaN or outside [0, 1].  n_samples == 0: DFH_OK and nothing
 * is launched (there is nothing to gate; the ungated twins are the calls that build a sample-less system or write empty sums). */
typedef struct dfh_gn_normal_gate {
    const float *normals;   /* n_views x H x W x 3 float32 (device), view-major, contiguous: dfh_depth_prep's layout.  Camera space of
                               each view, (0,0,0) = the pixel has no normal.  Need not be unit length. */
    double min_cos;         /* in [0, 1]: the smallest cosine between model and live normal that still passes */
} dfh_gn_normal_gate;
int dfh_gn_associate_gated(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_normal_gate *gate, void *stream);
int dfh_gn_build_gated(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_normal_gate *gate, void *stream);
int dfh_gn_solve_gated(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_normal_gate *gate,
                       const dfh_gn_solve_params *params, void *stream);

/* The landmark term: point-to-point rows for feature correspondences (opt-in: the calls above know nothing of it).  The data rows
 * n'.(x' - c) cannot see motion inside the surface; a landmark ties a canonical point p to a live 3-D target c with all three
 * components of x' - c (DynamicFusion section 6, VolumeDeform's sparse term).  The reference has no counterpart (its matches feed
 * its one point-to-plane term, core/fusion.py:282-285, 444-473).  Everything is fp64, operation by operation in this order, no
 * contraction.  For landmark l with its knn nodes nbr[l][.] and static blend weights weights[l][.] (knn = the problem's):
 *  1. x' = the landmark warped exactly as dfh_gn_associate warps a sample: b^ = the normalised static blend of its node DQs,
 *     x' = dqb_warp(lw_dq, f32(dqb_warp(b^, f32(p)))).
 *  2. d_a = x'_a - c_a (a = 0, 1, 2);  q = (d_0*d_0 + d_1*d_1) + d_2*d_2.
 *  3. s2 = weight * conf[l] (conf == NULL: 1).  The landmark is ACTIVE iff valid[l] != 0 (valid == NULL: 1), s2 > 0, q < +inf (a NaN
 *     fails both) and (max_dist <= 0 or q <= max_dist*max_dist).  An inactive landmark adds nothing.
 *  4. vector Huber on |d|: if huber_delta > 0 and q > huber_delta*huber_delta: n = sqrt(q), obj = s2*huber_delta*(n - 0.5*huber_delta),
 *     sc = sqrt(s2)*sqrt(huber_delta/n); otherwise obj = 0.5*s2*q, sc = sqrt(s2).
 *  5. three rows, a = 0, 1, 2: residual sc*d_a, Jacobian sc*J_a, J_a = the data row's gradient (oracle/gn_np.py
 *     data_residual_jacobian) with the warped normal replaced by the constant axis e_a and its normal-rotation (H) term dropped:
 *     U = pure(vec(rl* e_a rl)), g_r = -2 (U r^ P + U d^), g_d = 2 U r^, then the same projection off b^, the same division by
 *     |b|_8 and the same per-node products.
 *  6. vals += J^T J, rhs += J^T r, cost_count[0] += sum of obj; cost_count[1] (the valid SAMPLES) is left alone.  Node pairs that
 *     are no block of the pattern are dropped silently, as for samples.
 * Landmarks arrive sorted by node tuple; their plan is the data plan's (dfh_gn_plan_count / dfh_gn_plan_build on the landmarks' nbr
 * against the problem's pattern), `partial` sized as dfh_gn_problem.partial is.  No floating-point atomics: the same bits every
 * run.  Restated in tests/landmark_np.py.
 * dfh_gn_add_landmarks: adds the term to the system any build left in the problem (reads node_dq, lw_dq, knn, the pattern and
 * blk_upper; adds to vals / rhs / cost_count).  dfh_gn_solve_landmarks: dfh_gn_solve (the ungated depth term) with the term added
 * after every build, the rigid-mode steps' builds included -- the same bits as the separate calls; frame == NULL: the builds use
 * the problem's corr / valid.  DFH_E_BADARG (before any HIP call): what dfh_gn_build / dfh_gn_solve refuse, a null struct, n < 0, with
 * n > 0 a null pos / nbr / weights / target / run_id / partial / blk_ptr / node_ptr (or, with n_rows > 0, blk_ent / node_ent) or
 * n_rows < 1, weight negative or not finite, huber_delta negative or NaN, max_dist NaN.  n == 0 or weight == 0: DFH_OK, nothing is
 * launched by the term and the system is left as it is. */
typedef struct dfh_gn_landmarks {
    const double *pos;            /* n x 3 canonical positions (index space), sorted by node tuple */
    const int *nbr;               /* n x knn */
    const double *weights;        /* n x knn static blend weights */
    const double *target;         /* n x 3 live targets (index space) */
    const unsigned char *valid;   /* n, may be NULL (all valid) */
    const double *conf;           /* n, may be NULL (all 1) */
    int n;
    double weight, huber_delta, max_dist;
    const int *run_id;            /* the landmarks' plan, laid out as dfh_gn_problem's data plan */
    int n_rows;
    double *partial;
    const int *blk_ptr, *blk_ent, *node_ptr, *node_ent;
    unsigned char *active_out;    /* n, may be NULL: 1 iff the landmark was active (step 3) */
} dfh_gn_landmarks;
int dfh_gn_add_landmarks(const dfh_gn_problem *problem, const dfh_gn_landmarks *landmarks, void *stream);
int dfh_gn_solve_landmarks(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_landmarks *landmarks,
                           const dfh_gn_solve_params *params, void *stream);

/* The photometric term: one colour-consistency row per sample (opt-in: the calls above know nothing of it).  The data rows
 * n'.(x' - c) cannot see motion inside the surface, and landmarks need feature matches the caller has to bring; an RGB-D frame's
 * colour images constrain the tangential motion densely (VolumeDeform, KillingFusion): a canonical point with a reference
 * intensity ref (the luma of the colour volume, dfh_sample_colors) should project onto a live pixel of that intensity.  The
 * reference has no counterpart (it reconstructs geometry only).  Everything is fp64, operation by operation in this order, no
 * contraction.  For photo sample l with its knn nodes nbr[l][.] and static blend weights weights[l][.] (knn = the problem's), a
 * frame (the packed views, K, Kinv, scale, center, half; its max_dist is not read) and the views' colour images color[v] (K17's
 * format: uint8 [v][u][4] R, G, B, X of the depth maps' H x W, a HOST array of n_views device pointers as dfh_integrate_color takes):
 *  1. x' = the sample warped exactly as dfh_gn_landmarks step 1: x' = dqb_warp(lw_dq, f32(dqb_warp(b^, f32(p)))).
 *  2. for every view 0 .. n_views-1 in turn, the association's chain:
 *       pos  = scale*(x' - half) + center
 *       lpos = lw*[pos,1]  (l_i = ((lw_i0*pos_0 + lw_i1*pos_1) + lw_i2*pos_2) + lw_i3)
 *       (a, b, c) = K*lpos  (each (K_i0*l_0 + K_i1*l_1) + K_i2*l_2);  skipped if c == 0;  u = a/c, v = b/c  (IEEE divisions)
 *       visible iff 0 <= u < W-1 and 0 <= v < H-1 (a NaN fails)
 *       z = -depth[rint(v)][rint(u)] (round-half-even), valid iff z > 0; a z*u or z*v that is not finite passes nothing
 *       sd = ((Kinv_20*(z*u) + Kinv_21*(z*v)) + Kinv_22*(z*1.0)) - l_2;  the view PASSES iff fabs(sd) <= band_sd (a NaN fails)
 *  3. the sample's view is the passing view with the smallest fabs(sd): a view replaces the best so far iff its fabs(sd) is
 *     strictly smaller (the best starts at +inf), so ties go to the lowest index.
 *  4. intensity in that view: a pixel's Y = (double)(77*R + 150*G + 29*B) / 256.0 (exact);  i0 = (int)floor(u), j0 = (int)floor(v),
 *     fu = u - i0, fv = v - j0;  Y00 = Y[j0][i0], Y10 = Y[j0][i0+1], Y01 = Y[j0+1][i0], Y11 = Y[j0+1][i0+1];
 *       I  = (1-fv)*((1-fu)*Y00 + fu*Y10) + fv*((1-fu)*Y01 + fu*Y11)
 *       Iu = (1-fv)*(Y10-Y00) + fv*(Y11-Y01)
 *       Iv = (1-fu)*(Y01-Y00) + fu*(Y11-Y10)
 *     Iu, Iv are the exact derivatives of the bilinear interpolant inside the cell: no gradient image, no second pass.
 *  5. r = I - ref[l];  s2 = weight * conf[l] (conf == NULL: 1).  The sample is ACTIVE iff valid[l] != 0 (valid == NULL: 1), s2 > 0, a
 *     view passed, fabs(r) < +inf (a NaN ref fails) and (max_diff <= 0 or fabs(r) <= max_diff).  Scalar Huber on |r| (delta in
 *     intensity units), K16 step 4 with q = r*r: if huber_delta > 0 and q > huber_delta*huber_delta: n = sqrt(q),
 *     obj = s2*huber_delta*(n - 0.5*huber_delta), sc = sqrt(s2)*sqrt(huber_delta/n); otherwise obj = 0.5*s2*q, sc = sqrt(s2).
 *  6. the image gradient pulled back to index space, with R the 3x3 part of the view's lw:
 *       du_j = (K_0j - u*K_2j)/c,  dv_j = (K_1j - v*K_2j)/c,  h_j = Iu*du_j + Iv*dv_j          (j = 0, 1, 2: d I / d lpos)
 *       g_i  = scale*((h_0*R_0i + h_1*R_1i) + h_2*R_2i)                                        (i = 0, 1, 2: d I / d x')
 *     one row: residual sc*r, Jacobian sc*J, J = the landmark term's axis row (dfh_gn_landmarks step 5) with the axis e_a replaced
 *     by the vector g: U = pure(vec(rl* g rl)), then the same g_r, g_d, projection off b^, division by |b|_8 and per-node
 *     products.  g is held constant while the row is differentiated -- the Gauss-Newton linearisation of I(x'(xi)): the pixel, the
 *     cell and the view are not differentiated.
 *  7. vals += J^T J, rhs += J^T r, cost_count[0] += sum of obj; cost_count[1] (the valid SAMPLES) is left alone.  Node pairs that
 *     are no block of the pattern are dropped silently, as for samples.
 * The samples arrive sorted by node tuple with a plan laid out as dfh_gn_problem's data plan (the solver's own samples bring the
 * data plan itself; only `partial`, sized as dfh_gn_problem.partial is, must be the term's own).  No floating-point atomics: the
 * same bits every run.  Outputs (each may be NULL): active_out[l] = 1 iff active; view_out[l] = the sample's view, -1 when
 * inactive; resid_out[l] = the unscaled r, 0 when inactive.  Restated in tests/photometric_np.py.
 * dfh_gn_add_photometric: adds the term to the system any build left in the problem (reads node_dq, lw_dq, knn, the pattern and
 * blk_upper; adds to vals / rhs / cost_count); depth maps of either dtype.  dfh_gn_solve_photometric: dfh_gn_solve_landmarks'
 * schedule with the photometric term added after every build (after the landmark term where both are given), the rigid-mode
 * steps' builds included -- the same bits as the separate calls.  landmarks == NULL: no landmark term.  photo == NULL: the call
 * sequence of dfh_gn_solve_landmarks (of dfh_gn_solve when landmarks == NULL too); with photo the frame is required (DFH_F32 maps).
 * DFH_E_BADARG (before any HIP call): what dfh_gn_build / dfh_gn_solve refuse, a null struct, n < 0, with n > 0 a null pos / nbr /
 * weights / ref / run_id / partial / blk_ptr / node_ptr (or, with n_rows > 0, blk_ent / node_ent) or n_rows < 1, weight negative or
 * not finite, huber_delta negative or NaN, max_diff NaN, band_sd not > 0 (NaN refused, +inf allowed), a null frame (or one
 * dfh_gn_associate refuses), a null color or color[v].  n == 0 or weight == 0: DFH_OK, nothing is launched by the term and the
 * system is left as it is. */
typedef struct dfh_gn_photometric {
    const double *pos;            /* n x 3 canonical positions (index space), sorted by node tuple */
    const int *nbr;               /* n x knn */
    const double *weights;        /* n x knn static blend weights */
    const double *ref;            /* n reference intensities (0..255) */
    const unsigned char *valid;   /* n, may be NULL (all valid) */
    const double *conf;           /* n, may be NULL (all 1) */
    int n;
    double weight, huber_delta, max_diff, band_sd;
    const void *const *color;     /* HOST array of frame->n_views device pointers to H x W RGBX images */
    const int *run_id;            /* the samples' plan, laid out as dfh_gn_problem's data plan */
    int n_rows;
    double *partial;
    const int *blk_ptr, *blk_ent, *node_ptr, *node_ent;
    unsigned char *active_out;    /* n, may be NULL */
    int *view_out;                /* n, may be NULL */
    double *resid_out;            /* n, may be NULL */
} dfh_gn_photometric;
int dfh_gn_add_photometric(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_photometric *photo, void *stream);
int dfh_gn_solve_photometric(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_landmarks *landmarks,
                             const dfh_gn_photometric *photo, const dfh_gn_solve_params *params, void *stream);

/* Multi-GPU solve: what travels in the per-iteration all-reduce.  `system` = {J^T J blocks (n_blocks x 36) | J^T r (6 n_nodes) |
 * cost, count} as the builds write it; J^T J is symmetric, so only the blocks with col >= row are packed (then J^T r and
 * {cost, count}): (36 n_upper + 6 n_nodes + 2) doubles in `packed`, about 55 % of the system.  row_of[b] / col[b]: block b's
 * row and column node; src[b]: index among the packed blocks of the one that holds block b's data (its own, or its mirror's
 * when col < row: the unpack transposes it).  No reference counterpart (the reference has no collective). */
int dfh_gn_pack_upper(const double *system, const int *row_of, const int *col, const int *src, int n_blocks, int n_nodes, int n_upper,
                      double *packed, void *stream);
int dfh_gn_unpack_upper(double *system, const int *row_of, const int *col, const int *src, int n_blocks, int n_nodes, int n_upper,
                        const double *packed, void *stream);

/* The persistent PCG kernel (one launch per solve; its workgroups synchronise through grid-wide reductions) is used
 * when all its workgroups are co-resident: the occupancy query admits a workgroup per CU and the grid needs at most
 * one workgroup per CU.  That cannot be known when several PROCESSES time-share one GPU: such callers declare it with
 * dfh_pcg_set_mode(2) and every solve then takes the two-launches-per-iteration path (0 = auto, the default).
 * A barrier of the persistent kernel that does not complete within its spin bound (seconds) makes every workgroup
 * leave: x_out = NaN, node_dq untouched (the twist update of dfh_pcg_solve_update / dfh_gn_solve is all or nothing: the
 * workgroup that finishes last applies every row's step, and only if no barrier timed out and every x is finite -- after a
 * timed-out solve node_dq is what it was before that solve), and a per-device counter is bumped.  dfh_pcg_status() synchronises `stream`,
 * reads and clears that counter: DFH_OK, or DFH_E_TIMEOUT when a solve since the last call timed out
 * (*aborted_solves_out = how many; may be NULL).  Call it wherever the host synchronises anyway. */
int dfh_pcg_set_mode(int mode);
/* Which path a solve with n_nodes rows takes on the current device right now: 1 = the persistent single-reduction kernel,
 * 2 = two launches per iteration (the textbook recurrence; same iterates in exact arithmetic, not the same bits), < 0 = error.
 * Callers that compare runs bit for bit (N ranks against one GPU) compare runs of the same path. */
int dfh_pcg_path(int n_nodes);
int dfh_pcg_status(void *stream, long *aborted_solves_out);
/* The same answer for the solves that have COMPLETED, without touching the device when none of them timed out (the kernel
 * also sets a word of pinned host memory): for callers that have just synchronised for a reason of their own (a count
 * read back) and do not want a second device round trip per frame.  Falls back to dfh_pcg_status() when the word is set. */
int dfh_pcg_status_peek(void *stream, long *aborted_solves_out);

/* node_dq[a] <- exp(step * xi[a]) (x) node_dq[a]; exp = rotation exp(omega), translation v. */
int dfh_apply_twist(double *node_dq, const double *xi, int n_nodes, double step, void *stream);
/* node_dq[a] <- exp(factor * log(node_dq[a])), 0 <= factor <= 1: every node's rotation vector and translation scaled by factor
 * towards the identity (a decoupled scaling of the two; q and -q relax alike: the log is taken with w >= 0, rotation angles in
 * [0, pi]; a unit dual quaternion comes back; entries whose |q|^2 is not inside (1e-300, 1e300), zero or non-finite ones, are left
 * alone; factor = 1 launches nothing).  Restated in oracle/gn_np.relax_twists.  The composed frame loop calls it once
 * per frame after the TSDF update (pipeline.SlabFrame.step(relax=...)): Fusion.updateTSDF moves the canonical surface most of
 * the way to the live one every frame (core/fusion.py:180-190: the live sample weighs wi ~ tens against a canonical weight that
 * starts at the view count), so what the field carried is largely in the volume afterwards -- without this decay nothing ever
 * pulls a node back and the field random-walks.  No reference counterpart. */
int dfh_relax_twists(double *node_dq, int n_nodes, double factor, void *stream);
/* The rigid mode of a built system (dfh_gn_build: vals, rhs), solved on its own: all nodes share ONE twist xi --
 * (sum of all 6x6 blocks + lm_rel diag) xi = -(sum of all J^T r) -- which is applied to every node,
 * node_dq[a] <- exp(xi) (x) node_dq[a], and written to xi_out (6 doubles, may be NULL).  Block-Jacobi PCG truncated at ten
 * iterations hardly moves this mode (the regulariser does not penalise it, the preconditioner does not see it); the frame loop
 * takes two such steps, each behind a build, before its node iterations (pipeline.SlabFrame.step(global_iters=...)).  The
 * reference fits a global rigid motion first too (Fusion.solve, precompute_lw: core/fusion.py:356-365).  scratch: device
 * memory of dfh_gn_global_step_bytes() bytes, ZEROED by the caller once (the kernel leaves it ready for the next call); sums
 * are added in a fixed order: the same bits every run.  Restated in oracle/gn_np.global_step. */
/* The same rigid-mode step from a SUBSAMPLE of the data rows, without a built system (what the frame loop takes): every
 * `stride`-th 128-sample tile of the (sorted) samples is associated against the views' table and differentiated as in the builds
 * (same Huber weights); a sample's Jacobian for the shared twist is the sum of its knn node blocks; the regulariser is left out (a
 * common left twist only rotates its residuals).  n_steps steps, each three short launches (rows, the 29 sums -- 21 upper entries
 * of A_g, 6 of g_g, objective, valid count -- and solve + apply); xi_out (8 doubles, may be NULL): the last step's twist | its
 * objective | its valid-sample count.  scratch: dfh_gn_global_sampled_bytes(n_samples, stride) bytes.  Sums in a fixed order: the
 * same bits every run.  Of the problem it reads the samples, node_dq, n_nodes, lw_dq and huber_delta; the frame's maps may be
 * DFH_F32 or DFH_F64.  sums_out != NULL (n_steps = 1): only the 29 sums of THIS rank's samples are produced (32 doubles) -- the caller all-reduces them over ranks and calls dfh_gn_global_apply: every rank then applies the same twist.
 * Restated in oracle/gn_np.global_step_sampled. */
size_t dfh_gn_global_sampled_bytes(int n_samples, int stride);
int dfh_gn_global_sampled(const dfh_gn_problem *problem, const dfh_gn_frame *frame, int stride, double lm_rel, int n_steps,
                          double *xi_out, double *sums_out, void *scratch, size_t scratch_bytes, void *stream);
/* dfh_gn_global_sampled with the volume data term: the samples of every `stride`-th tile are associated by the cell evaluation of
 * dfh_gn_associate_volume (a DFH_F32 or DFH_F64 live volume, knn 1..8) instead of against the views' table; everything else -- the
 * rows, the sums and their order, scratch, xi_out, sums_out with n_steps = 1 followed by dfh_gn_global_apply -- is that call's
 * contract.  A sample beyond n_samples touches no voxel.  n_steps == 0: DFH_OK, nothing is checked further or launched. */
int dfh_gn_global_sampled_volume(const dfh_gn_problem *problem, const dfh_gn_volume_term *term, int stride, double lm_rel, int n_steps,
                                 double *xi_out, double *sums_out, void *scratch, size_t scratch_bytes, void *stream);
/* dfh_gn_global_sampled through the normal gate (dfh_gn_normal_gate above): float32 or float64 maps, knn 1..8; the rows, the sums
 * and their order, scratch, xi_out and sums_out are that call's.  n_steps == 0: DFH_OK, nothing is checked further or launched. */
int dfh_gn_global_sampled_gated(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_normal_gate *gate, int stride,
                                double lm_rel, int n_steps, double *xi_out, double *sums_out, void *scratch, size_t scratch_bytes, void *stream);
int dfh_gn_global_apply(const double *sums29, double lm_rel, int n_nodes, double *node_dq, double *xi_out, void *stream);
size_t dfh_gn_global_step_bytes(void);
int dfh_gn_global_step(const double *vals, int n_blocks, const double *rhs, int n_nodes, double lm_rel, double *node_dq, double *xi_out,
                       void *scratch, size_t scratch_bytes, void *stream);

/* ---- surface samples for the solve (stand-in for marching cubes, core/fusion.py:554-568) -----------
 * Every band voxel (w > 0, |T| < band, both comparisons strict and false for NaN; T in voxel units as fuseDepths stores it)
 * whose TSDF gradient g has a length |g| that is finite and > 1e-6 yields one sample.  Everything in fp64, no fused
 * multiply-add, operations in the order written (restated in numpy by tests/extract_np.py):
 *  - g_a = (T[hi] - T[lo]) / (hi - lo) along each axis a, with lo = max(i - 1, 0) and hi = min(i + 1, n - 1) inside the slab
 *    (central differences, one-sided at its faces), and g_a = 0 on an axis that is one voxel thick;
 *  - |g| = sqrt((gx gx + gy gy) + gz gz).  A NaN or infinite neighbour makes |g| NaN or infinite: no sample, so no
 *    non-finite number reaches the outputs (|T| < band keeps T itself finite);
 *  - normal n = g / |g|; position = voxel centre - (T / max(|g|, 1)) n (one Newton step, never longer than |T|; global index
 *    space: plane 0 of the buffer is global plane x0, which is added to the centre before the step is subtracted).
 * Samples come out in voxel order, deterministically.
 *   dfh_surface_count : per-block counts + exclusive scan into `workspace`, *total_out (device) = count
 *   dfh_surface_emit  : writes min(total, capacity) samples (n x 3 fp64 each); uses the same workspace.  capacity < total:
 *                       an even subsample in voxel order (sample i is kept iff it is the first with slot floor(i * capacity /
 *                       total), and stored in that slot), not a prefix. */
size_t dfh_surface_workspace_bytes(const int res[3]);
int dfh_surface_count(const void *tsdf, const void *tsdf_w, int vol_dtype, const int res[3], double band, void *workspace,
                      size_t workspace_bytes, long *total_out, void *stream);
int dfh_surface_emit(const void *tsdf, const void *tsdf_w, int vol_dtype, const int res[3], int x0, double band,
                     const void *workspace, double *pos_out, double *nrm_out, long capacity, void *stream);

/* ---- marching cubes: `_vertices` / `_faces` / `_normals` from a TSDF volume --------------------------
 * Replaces measure.marching_cubes_lewiner(volume, level, step_size, allow_degenerate=False) as called at
 * core/fusion_dm.py:319-331,342 and core/fusion.py:554-568 (skimage 0.13.1, a third-party dependency
 * that is not vendored).  Vertices sit on the edges of the step-subsampled lattice at the linearly
 * interpolated crossing of `level` (array-index coordinates, fp32 like skimage's), unit normals point
 * down the gradient (central differences on the lattice), faces are wound with their right-hand normal
 * up the gradient, zero-area faces are dropped -- the conventions of the reference's own output
 * meshes/original.obj.  Triangle choice inside a cube and the output order are this library's
 * (deterministic: vertices by owning lattice point then axis, faces by cube then table order).
 *   dfh_mc_count : totals_out[0] = vertices, [1] = faces, [2] = z rows (tiles) that emit anything
 *                  (3 device longs); fills `workspace`
 *   dfh_mc_emit  : writes min(total, capacity) vertices (x3 fp32), normals (x3 fp32), values (max of the
 *                  edge's two samples, may be NULL) and faces (x3 int32); same workspace, after dfh_mc_count.
 *                  n_active_tiles = totals_out[2] launches only those tiles; < 0 visits every tile. */
size_t dfh_mc_workspace_bytes(const int res[3], int step);
int dfh_mc_count(const void *vol, int vol_dtype, const int res[3], int step, double level, void *workspace,
                 size_t workspace_bytes, long *totals_out, void *stream);
int dfh_mc_emit(const void *vol, int vol_dtype, const int res[3], int step, double level, void *workspace,
                size_t workspace_bytes, float *verts, float *normals, float *values, int *faces, long cap_verts, long cap_faces,
                long n_active_tiles, void *stream);
/* The reference's vertex order on top of dfh_mc_emit's output: skimage numbers vertices as its faces create
 * them and flips the face rows afterwards, i.e. ids increase with first use when rows are read right-to-left
 * (meshes/original.obj).  Renumbers accordingly (faces rewritten in place, vertex arrays copied to *_out in
 * the new order), drops vertices no face uses; *used_out (device) = vertices kept. */
size_t dfh_mc_reorder_workspace_bytes(long n_verts, long n_faces);
int dfh_mc_reorder(const float *verts_in, const float *normals_in, const float *values_in, int *faces, long n_verts, long n_faces,
                   float *verts_out, float *normals_out, float *values_out, long *used_out, void *workspace,
                   size_t workspace_bytes, void *stream);

/* ---- rasterizer: depth / face-id / normal maps of a triangle mesh in V views (no reference counterpart) -----------------
 * The model-to-frame prediction of DynamicFusion: the (warped) model as the cameras would see it.  One mesh, V views of
 * H x W pixels (1 <= V <= 16), one call.  Semantics (restated in numpy by tests/render_np.py; everything in fp64, no
 * fused multiply-add, operations in the order written):
 *  - vertices (n_verts x 3 fp64) are in voxel-index space; world w = scale * (p - half) + center (K1's map,
 *    dfh_integrate_depth); camera c = R w + t with lw = [R | t] (3 x 4 row-major per view, world -> camera), each row
 *    summed as ((r0 w0 + r1 w1) + r2 w2) + t.
 *  - K (3 x 3 row-major per view) must be upper-triangular with last row (0, 0, 1) (else DFH_E_BADARG);
 *    u = (K00 c0 + K01 c1 + K02 c2) / c2, v = (K11 c1 + K12 c2) / c2.  Pixel centres sit at integer (u, v) (the
 *    convention of scene.render_depth); outputs are indexed [view][v][u].
 *  - A triangle (faces: n_faces x 3 int32) draws nothing in a view if a vertex index lies outside [0, n_verts), any vertex
 *    has c2 <= znear or a non-finite u / v, or its area A = E01(u2, v2) is 0 or not finite, where
 *    E_ab(x, y) = (x - u_a)(v_b - v_a) - (y - v_a)(u_b - u_a).  There is NO clipping: a triangle crossing znear is dropped.
 *  - Pixels tested: the bounding box [ceil(min u), floor(max u)] x [ceil(min v), floor(max v)] clamped to the image.
 *    Edge values e0 = E12, e1 = E20, e2 = E01 at the pixel centre, each evaluated from the lexicographically smaller (u, v)
 *    end point of its edge (E_ab as written if (u_a, v_a) < (u_b, v_b), else -E_ba) so that triangles sharing an edge get
 *    exactly opposite values.  Covered: all three have A's sign or are 0 (inclusive, no back-face culling: a closed mesh is
 *    watertight).  lambda_i = e_i / A; s = (lambda0 / z0 + lambda1 / z1) + lambda2 / z2 (z_i = c2 of vertex i); the pixel
 *    is dropped unless s > 0 and (float)(1 / s) is finite; z = (float)(1 / s), perspective-correct.
 *  - Z-buffer: one uint64 key per pixel, (bits of z) << 32 | face, reduced with a 64-bit atomicMin (positive floats order
 *    like their bit patterns): the nearest surface wins, ties go to the lowest face id, independent of scheduling.
 *  - Resolve: depth (V x H x W fp32) = -z (the reference's storage convention: negative, 0 = no surface, so a rendered map
 *    can be fused like a camera's); face (V x H x W int32) = winning face, -1 where none; normal (V x H x W x 3 fp32, only
 *    with normals, n_verts x 3 fp64): m = (a0 n0 + a1 n1) + a2 n2 with a_i = lambda_i / z_i of the winning face, rotated
 *    into the camera frame by R and normalised (0 where there is no surface or the vector is 0).
 * dfh_render_raster clears the key buffer of `workspace` (dfh_render_workspace_bytes(n_views, H, W, n_faces) bytes: the keys
 * and the list of triangles whose box exceeds 64 pixels, which a second launch rasterises workgroup by workgroup) and fills it;
 * dfh_render_resolve reads it and writes the maps (same mesh, views and map as the raster call).  Both only enqueue on
 * `stream`; K / lw / center are host arrays read during the call.
 * Workspace layout (each part starts 16-byte aligned): first the keys, n_views x H x W uint64, indexed [view][v][u]; then ONE
 * uint32, the number of listed (triangle, view) pairs, i.e. those that draw and whose clamped box exceeds 64 pixels; then the
 * list, up to n_views x n_faces uint32 entries view * n_faces + face in no particular order.  dfh_render_raster resets the
 * count and the keys on every call, so a workspace may be reused as it is; after the call the count and the list can be read
 * back (tests/test_gpu_raster_edges.py does, to see which path drew a triangle). */
size_t dfh_render_workspace_bytes(int n_views, int H, int W, long n_faces);
int dfh_render_raster(const double *verts, long n_verts, const int *faces, long n_faces, int n_views, const double *K, const double *lw,
                      int H, int W, double scale, const double center[3], double half, double znear, void *workspace,
                      size_t workspace_bytes, void *stream);
int dfh_render_resolve(const double *verts, const double *normals, long n_verts, const int *faces, long n_faces, int n_views,
                       const double *K, const double *lw, int H, int W, double scale, const double center[3], double half, double znear,
                       const void *workspace, size_t workspace_bytes, float *depth_out, int *face_out, float *normal_out, void *stream);

/* ---- visible-surface samples: the rendered model as the warp solve's sample set (no reference counterpart) --------------
 * DynamicFusion's data term is model-to-frame: every pixel the rendered (warped) model covers gives one point-to-plane row,
 * the CANONICAL point and normal of the surface visible there.  After dfh_render_raster (no resolve pass is needed: only the
 * key buffer of `workspace` and the mesh are read) these calls turn the covered pixels into samples.  verts / faces / views /
 * H / W / scale / center / half / znear are the raster call's; canon_pos and canon_nrm (n_verts x 3 fp64) are per-vertex
 * attributes of the canonical mesh (the unwarped vertices and normals; any arrays will do).  Semantics (restated in numpy by
 * tests/render_samples_np.py; everything in fp64, no fused multiply-add, operations in the order written):
 *  - Lattice pixels: (view, y, x) with x % stride == 0 and y % stride == 0 (stride >= 1), enumerated view-major, then y,
 *    then x.  A lattice pixel yields a sample iff its key is not the empty key; `total` is the number of such pixels.
 *  - Weights: f = the low 32 bits of the key; lambda_i, z_i = the rasterizer's barycentric weights and vertex depths of
 *    face f in that view at (x, y) (the set-up and edge values above); a_i = lambda_i / z_i; s = (a0 + a1) + a2;
 *    b_i = a_i / s.
 *  - pos[c] = (b0 P0[c] + b1 P1[c]) + b2 P2[c] with P_i the rows of canon_pos at the face's vertices.
 *  - m[c] = (b0 N0[c] + b1 N1[c]) + b2 N2[c] likewise from canon_nrm; len = sqrt((m0 m0 + m1 m1) + m2 m2);
 *    nrm = m / len if len > 0 and finite, else (0, 0, 0).  canon_nrm and nrm_out may both be NULL (nrm_out without canon_nrm:
 *    DFH_E_BADARG).
 *  - pixel (int64) = (view * H + y) * W + x.
 *  - Samples come out in lattice order, deterministically (per-workgroup counts, an exclusive scan, ordered emission: no
 *    atomics).  capacity < total: dfh_surface_emit's even subsample -- sample i is kept iff it is the first with slot
 *    floor(i * capacity / total), and stored in that slot; never a prefix.  Rows at and beyond min(total, capacity) are not
 *    written; nothing covered (or n_faces == 0): DFH_OK, count 0, no row written.
 *   dfh_render_samples_count : fills `scan_workspace` (dfh_render_samples_workspace_bytes(n_views, H, W, stride) bytes; 0 for
 *                              bad sizes) from the keys; *total_out = total by ONE plain store of the last launch (device or
 *                              pinned host memory, like dfh_surface_count's)
 *   dfh_render_samples_emit  : pos_out / nrm_out (capacity x 3 fp64) and pixel_out (capacity int64), after the count call
 *                              with the same workspaces and stride.  pixel_out is written first and read back as the list of
 *                              kept samples: one lane per kept sample computes the rows.
 * Both only enqueue on `stream`.  DFH_E_BADARG before any HIP call: null required pointers, stride < 1, sizes the render
 * calls refuse, capacity < 0, a workspace smaller than its size query. */
size_t dfh_render_samples_workspace_bytes(int n_views, int H, int W, int stride);
int dfh_render_samples_count(int n_views, int H, int W, long n_faces, int stride, const void *workspace, size_t workspace_bytes,
                             void *scan_workspace, size_t scan_workspace_bytes, long *total_out, void *stream);
int dfh_render_samples_emit(const double *verts, const double *canon_pos, const double *canon_nrm, long n_verts, const int *faces,
                            long n_faces, int n_views, const double *K, const double *lw, int H, int W, double scale, const double center[3],
                            double half, double znear, int stride, const void *workspace, size_t workspace_bytes,
                            const void *scan_workspace, size_t scan_workspace_bytes, double *pos_out, double *nrm_out, long *pixel_out,
                            long capacity, void *stream);

/* ---- K12  depth preprocessing: bilateral filter, live normal map, flying-pixel mask ----------------------------------------
 * The first stage of KinectFusion / DynamicFusion, which the reference does not have: every depth map of a frame is smoothed,
 * back-projected, given a normal map and stripped of the pixels no surface normal can be computed for.  The cleaned maps keep
 * the convention every other entry point reads (negative depth, 0 = no measurement).
 * All arithmetic is float32 with ONE rounding per operation (no contraction, IEEE division and square root, subnormals kept),
 * so that an element-wise float32 numpy restatement (tests/depth_prep_np.py) agrees bit for bit; that is why the range weight
 * is a caller's table and not a device exp.
 *
 * Per view v, D = depth[v] (H x W, only read; a float64 value is rounded to nearest-even float32 at load).
 *   valid(d)  <=>  d is finite and d < 0          (-0.0, 0, positive values, NaN, +-inf: "no measurement")
 * Stage A, bilateral filter, r = radius, s = (float)range_scale; centre d = D[y][x]:
 *   centre not valid            -> F = 0
 *   r == 0                      -> F = d            (no table is read)
 *   otherwise num = den = 0; for dy = -r..r (outer), dx = -r..r (inner), in that order, every tap e = D[y+dy][x+dx] that lies
 *   inside the image and is valid:
 *     delta = e - d;  q = (delta*delta)*s;  the tap counts iff q < (float)n_lut;  i = (int)q (truncation)
 *     w = spatial[(dy+r)*(2r+1) + (dx+r)] * range_lut[i];  num = num + w*e;  den = den + w
 *   F = num / den if den > 0, else 0.
 * Stage B, vertex and normal: Kf = float32(Kinv), J = (float)max_jump, m2 = (float)min_cos * (float)min_cos; x, y are the
 * float32 values of the pixel's integer indices:
 *   rho_i(x, y) = (Kf[i][0]*x + Kf[i][1]*y) + Kf[i][2];   P_i = z*rho_i with z = -F
 * Pixel (y, x) HAS A NORMAL iff valid(F[y][x]); its four neighbours (y, x+-1), (y+-1, x) lie inside the image, are valid in F
 * and have |F_nb - F| <= J; and with a = P(y,x+1) - P(y,x-1), b = P(y+1,x) - P(y-1,x):
 *   n0 = a1*b2 - a2*b1;  n1 = a2*b0 - a0*b2;  n2 = a0*b1 - a1*b0;  l2 = (n0*n0 + n1*n1) + n2*n2;  l2 > 0 and finite;
 *   nh = n / sqrt(l2) (three divisions);  c = (nh0*P0 + nh1*P1) + nh2*P2 at the centre;  c > 0: nh = -nh, c = -c (the normal
 *   faces the camera);  pp = (P0*P0 + P1*P1) + P2*P2;  kept iff c*c >= m2*pp.
 * Outputs (device float32; either may be NULL, not both):
 *   normals (n_views, H, W, 3): nh, or zeros where the pixel has no normal
 *   clean   (n_views, H, W)   : F if mask == 0 or the pixel has a normal, else 0.  mask = 1 removes silhouette ("flying")
 *                               pixels, isolated pixels, pixels seen at a grazing angle and the one-pixel image border.
 * One launch for all views; the filtered map never goes through memory.  The outputs must not alias an input (the kernel reads
 * halos that other workgroups write: in-place use is not supported).
 * DFH_E_BADARG before any launch: a null params / depth array / depth[v]; n_views outside 1..16; a dtype other than DFH_F32 /
 * DFH_F64; H or W < 2 or H*W >= 2^31; radius outside 0..8; spatial or range_lut NULL with radius > 0; n_lut outside 1..4096;
 * range_scale not finite or <= 0; max_jump not finite or < 0; min_cos outside [0, 1]; mask not 0 or 1; both outputs NULL; an
 * output equal to one of the input pointers.
 * dfh_depth_prep_tile: the kernel's output tile (rows, columns) per workgroup, for tests that put image sizes on its edges. */
typedef struct dfh_depth_prep_params {
    int n_views;                  /* 1..16 */
    const void *const *depth;     /* HOST array of n_views device pointers, H x W row-major */
    int depth_dtype, H, W;        /* DFH_F32 | DFH_F64; H, W >= 2 */
    double Kinv[9];
    int radius;                   /* 0..8 */
    const float *spatial;         /* DEVICE (2r+1)^2, NULL allowed iff radius == 0 */
    const float *range_lut;       /* DEVICE n_lut,    NULL allowed iff radius == 0 */
    int n_lut;                    /* 1..4096 */
    double range_scale;           /* finite, > 0 */
    double max_jump;              /* finite, >= 0 */
    double min_cos;               /* 0..1 */
    int mask;                     /* 0 | 1 */
} dfh_depth_prep_params;
int dfh_depth_prep(const dfh_depth_prep_params *p, float *clean, float *normals, void *stream);
int dfh_depth_prep_tile(int tile_hw[2]);

/* ---- K14  descriptor correspondences: exact nearest neighbour in feature space -------------------------------------------------
 * The search of the reference's CNN branch (core/fusion.py:282-285): `KDTree(l_feats).query(s_feats[idx])` on the float64
 * copies of float32 descriptors, squared (no square root), with the tie rule the KD-tree leaves open made explicit.
 * query (n_query, dim) and base (n_base, dim): float32, row-major, device.  All arithmetic of the definition is fp64 with ONE
 * rounding per operation (no contraction), so that tests/descriptors_np.py agrees bit for bit:
 *   t_c      = (double)query[q][c] - (double)base[l][c]
 *   d2(q, l) = (((t_0*t_0) + t_1*t_1) + ...) + t_{dim-1}*t_{dim-1}            channels in ascending order
 *   the pair (q, l) COUNTS iff d2(q, l) is finite (float32 inputs cannot overflow the sum: iff neither row holds a NaN or an
 *   infinity)
 *   idx_out[q] = the counting l with the smallest d2(q, l), the LOWEST such l on exact ties;  d2_out[q] = that d2
 *   a query with no counting pair: idx_out[q] = -1, d2_out[q] = +inf.
 * Two paths give these same bits (csrc/dfh_descriptors.hip, DESIGN K14): the exact kernel evaluates every pair; the fast path
 * filters with a float32 score on the matrix cores, keeps every base row inside a proven guard band of the smallest score
 * and evaluates the definition on those.  Option nd_path: unset = the library decides by size, 1 = the exact kernel, 2 = the
 * fast path (any other set value: DFH_E_BADARG); dfh_nearest_descriptors_path reports the path a call of that size takes
 * (1 or 2).
 * d2_out may be NULL.  stats_out (device, 2 longs) may be NULL: [0] = pairs the fast path re-evaluated with the definition,
 * [1] = queries handed to the exact kernel (the exact path: 0 and n_query).
 * workspace: dfh_nearest_descriptors_workspace_bytes(n_query, n_base, dim) bytes of device memory, 16-byte aligned, read and
 * written by the fast path only (the exact path ignores it, NULL allowed there); the size is 0 for unusable sizes and for
 * n_query == 0.  Only enqueues on `stream`.
 * n_query == 0: DFH_OK before any launch.  DFH_E_BADARG before any HIP call: dim outside 1..64; n_base outside [1, 2^31);
 * n_query outside [0, 2^31); a bad nd_path; null query / base / idx_out; on the fast path a null, misaligned or too small
 * workspace. */
size_t dfh_nearest_descriptors_workspace_bytes(long n_query, long n_base, int dim);
int dfh_nearest_descriptors_path(long n_query, long n_base, int dim);
int dfh_nearest_descriptors(const float *query, long n_query, const float *base, long n_base, int dim, int *idx_out, double *d2_out,
                            long *stats_out, void *workspace, size_t workspace_bytes, void *stream);
/* dfh_nearest_descriptors_tile: tile[0], tile[1] = queries and base rows per workgroup step of the fast path's score kernel,
 * tile[2] = queries per workgroup of the exact kernel, tile[3] = candidate slots per query (more candidates: the exact kernel);
 * for tests that put sizes on those edges. */
int dfh_nearest_descriptors_tile(int tile[4]);

/* ---- K15  rendered-view descriptors: vertex ids, the network's input image, features pooled onto vertices --------------------
 * The reference's compute_correspondence (core/sdf.py:95-150) without its network: the mesh is rendered from a ring of cameras
 * with a vertex id in every pixel, each depth buffer becomes an 8-bit image, a per-pixel feature network (the caller's) runs on
 * the images, and every vertex takes the mean of the features of its pixels over all views.
 *
 * dfh_render_vertex_ids: after dfh_render_raster with the same mesh, views and workspace (as dfh_render_samples_* are).
 * Semantics (restated in numpy by tests/pool_np.py; fp64 unless said otherwise, no fused multiply-add, operations in the order
 * written).  For each pixel whose key is not the empty key:
 *  - f = the low 32 bits of the key, d = the float32 in its high bits (the camera depth z of the raster pass).
 *  - lambda_i, z_i = the rasterizer's barycentric weights and vertex depths of face f in that view at the pixel (the set-up and
 *    edge values above); a_i = lambda_i / z_i, the perspective-correct coordinates up to a common factor.
 *  - The winner is the reference's fragment-shader rule, i = (a0 > a1 && a0 > a2) ? 0 : (a1 > a2 ? 1 : 2): the corner with the
 *    largest coordinate; a tie between 0 and 1 goes to 1, every tie that involves corner 2 at the top goes to 2.
 *    vid = faces[f][i].
 *  - image, in float32 with one rounding per operation, zf = (float)zfar_img, zn = (float)znear_img:
 *    g = ((zf - d) / (zf - zn)) * 255, image = (uint8)g truncated toward zero (and clamped to [0, 255]: the float32 images of
 *    the bounds can put g a rounding outside).  The reference's expression on a GL depth buffer is algebraically the same.
 * A pixel whose key is empty, or whose d lies outside [znear_img, zfar_img] (compared in fp64), gets vid = -1 and image = 0
 * (the reference's background also maps to 0).  GL clips such fragments and shows what lies behind them; that is not
 * reproduced.  vid_out: V x H x W int32; image_out: V x H x W uint8, may be NULL.  Only enqueues on `stream`.
 * DFH_E_BADARG before any HIP call: null required pointers, sizes the raster call refuses, a workspace smaller than its size
 * query, zfar_img <= znear_img or either of them not finite. */
int dfh_render_vertex_ids(const double *verts, long n_verts, const int *faces, long n_faces, int n_views, const double *K, const double *lw,
                          int H, int W, double scale, const double center[3], double half, double znear, const void *workspace,
                          size_t workspace_bytes, double znear_img, double zfar_img, int *vid_out, unsigned char *image_out, void *stream);

/* dfh_pool_features: the ordered segmented mean (core/sdf.py:138-149).  vid (n_pixels int32) and feat (n_pixels x dim float32,
 * row-major) are device arrays; any id outside [0, n_verts) means "no vertex".  For every vertex v (restated in numpy by
 * tests/pool_np.py):
 *   cnt_out[v]     = the number of p with vid[p] == v
 *   acc            = +0.0f;  acc = acc + feat[p][c] over those p in ASCENDING order, float32, one rounding per addition
 *   feat_out[v][c] = acc / (float)cnt_out[v] (an IEEE float32 division) if cnt_out[v] > 0, else +0.0f
 * NaN and infinities propagate as the additions make them.  The output is a function of the input alone, bit-identical from
 * run to run: no floating-point atomic; one integer atomic per pixel counts and hands out a slot, every segment is then put into ascending pixel
 * order (in LDS up to tile[2] entries, by an ordered walk over vid beyond that) before one lane per channel sums it.
 * feat_out: n_verts x dim float32; cnt_out: n_verts int32.  workspace: dfh_pool_features_workspace_bytes(n_pixels, n_verts)
 * bytes of device memory, 16-byte aligned (0 for unusable sizes and when either count is 0: no workspace is needed then).
 * Only enqueues on `stream`, no host synchronisation.  n_pixels == 0: DFH_OK, zeros and cnt = 0 written.
 * DFH_E_BADARG before any HIP call: dim outside 1..64; n_pixels or n_verts negative or >= 2^31; null vid / feat (with pixels),
 * null feat_out / cnt_out (with vertices); a null, misaligned or too small workspace (with both). */
size_t dfh_pool_features_workspace_bytes(long n_pixels, long n_verts);
int dfh_pool_features(const int *vid, const float *feat, long n_pixels, int dim, long n_verts, float *feat_out, int *cnt_out,
                      void *workspace, size_t workspace_bytes, void *stream);
/* dfh_pool_features_tile: tile[0] = pixels per workgroup of the count and scatter passes, tile[1] = vertices per workgroup of
 * the scan, tile[2] = the longest segment ordered in LDS (longer ones take the ordered walk), tile[3] = pixels per step of
 * that walk; for tests that put sizes on those edges. */
int dfh_pool_features_tile(int tile[4]);

/* ---- K17  colour: a per-voxel colour volume fused through the warp field, colours sampled onto mesh vertices -----------------
 * No reference counterpart (the reference reconstructs geometry only).  The colour volume C is float32 [x][y][z][4] over a slab's
 * planes [x0, x1), z fastest, one aligned 16-byte pack (r, g, b, wc) per voxel: r, g, b running means in [0, 255], wc the colour
 * weight (0 = never coloured).  It is float32 whatever the TSDF volume's dtype.  A colour image belongs to one depth map and has
 * its H x W: uint8 [v][u][4], bytes R, G, B, X (X is ignored): a pixel is one dword.
 *
 * dfh_integrate_color.  cvol->slab must equal vol->slab; vol is only read.  Everything is fp64 without contraction.  For every
 * voxel i = (x, y, z) of the slab:
 *  1. canonical gate, before anything else: t = T[i], w = w[i], read in the volume's dtype and widened to double; the voxel is
 *     live iff w > 0 and fabs(t) <= band_vox (a NaN fails).  A voxel that is not live is not warped, not projected, and its C is
 *     neither read nor written.
 *  2. position: nodes == NULL: q = i exactly.  Otherwise q is K1w's q (dfh_integrate_depth_dqb above), bit for bit: the knn nearest
 *     nodes (searched in the brick's candidate list, or the stored indices, clamped to n_nodes - 1), the Gaussian weights, b^ and
 *     q = dqb_warp(lw_dq, float32(dqb_warp(b^, i))).
 *  3. for every view 0 .. n_views-1 in turn, K1w's chain:
 *       pos  = scale*(q - tsdf_res/2) + center
 *       lpos = lw*[pos,1];  (u,v) = (K*lpos)_{0,1}/(K*lpos)_2, skipped if (K*lpos)_2 == 0
 *       visible iff 0<=u<W-1 and 0<=v<H-1;  (ui, vi) = (rint(u), rint(v)) (round-half-even)
 *       z = -depth[vi][ui], valid iff z>0; a z*u or z*v that is not finite passes nothing
 *       sd = (Kinv*(z*[u,v,1]))_2 - lpos_2;  passes iff sd > -tdist   (tdist in the depth maps' units)
 *     then the view gate fabs(sd) <= band_sd (the occlusion and free-space test, in the depth maps' units).  A view that passes
 *     reads pix = color[view][vi][ui] and updates
 *       c_a <- (float)(((double)c_a * (double)wc + (double)pix_a) / ((double)wc + 1.0))   for a = r, g, b
 *       wc  <- (float)min((double)wc + 1.0, wmax)
 *     every stored component rounded to float32 after every view: n_views views in one call equal n_views one-view calls bit for bit.
 *  4. C[i] is loaded once, when the first view passes, and stored once, only if a view passed.
 * workspace (with nodes): the buffer of dfh_fuse_volume_dqb / dfh_integrate_depth_dqb.  This call never builds candidate lists and
 * never stores indices: the lists must have been built for these node positions, this knn and this slab by
 * dfh_dqb_build_candidates or by a rebuilding dfh_fuse_volume_dqb / dfh_integrate_depth_dqb call on the same buffer;
 * use_stored_indices != 0 reads the index region those calls filled (the buffer must have one).  Nothing in the workspace is
 * written: the weight region is not touched and the library's note of which dfh_fuse_volume_dqb path wrote it stays.
 * DFH_E_BADARG before any HIP call for what dfh_integrate_depth_dqb refuses of its volume, views and (when given) nodes, and: a
 * null cvol, rgbw, color or color[v]; cvol->slab != vol->slab; band_vox or band_sd not > 0 (NaN refused, +inf allowed); wmax < 1;
 * nodes and lw_dq not both null or both non-null; with nodes a workspace smaller than dfh_dqb_workspace_bytes(); use_stored_indices
 * without nodes or with a buffer that has no index region.  An empty slab or n_views == 0: DFH_OK, no launch.
 *
 * dfh_sample_colors: the colour of n points (device fp64 n x 3, GLOBAL index space), e.g. mesh vertices.  Per point p:
 *  - invalid (rgb = 0, valid = 0) if a coordinate is not finite or lies outside [0, res_a - 1];
 *  - i0_a = min((int)floor(p_a), res_a - 2), clamped at 0 for res_a == 1; f_a = p_a - i0_a;
 *  - the eight corners in the order (dx, dy, dz) = 000, 001, 010, ..., 111; a corner's trilinear weight tw = (wx*wy)*wz, each
 *    factor (1 - f_a) or f_a; a corner counts only if it lies in the grid, its plane in [x0, x1), and its wc > 0;
 *  - S = sum tw, rgb_a = (float)((sum tw*c_a) / S), both sums fp64, sequential in corner order; S == 0: invalid.
 * rgb_out: n x 3 float32; valid_out: n uint8.  DFH_E_BADARG before any HIP call: a null cvol, a bad slab, n < 0 or >= 2^31, with
 * n > 0 a null points, rgb_out or valid_out, or a null rgbw with a non-empty slab.  n == 0: DFH_OK, no launch. */
typedef struct dfh_color_volume { float *rgbw; dfh_slab slab; } dfh_color_volume;
int dfh_integrate_color(const dfh_color_volume *cvol, const dfh_volume *vol, const dfh_depth_views *views,
                        const void *const *color /* HOST array of n_views device pointers */, const dfh_nodes *nodes /* NULL: no warp */,
                        const double lw_dq[8] /* NULL iff nodes == NULL */, double tdist, double band_vox, double band_sd, double wmax,
                        void *workspace, size_t workspace_bytes, int use_stored_indices, void *stream);
int dfh_sample_colors(const dfh_color_volume *cvol, const double *points, long n, float *rgb_out, unsigned char *valid_out,
                      void *stream);

/* ---- K19  RGB-D ingest: raw depth and unregistered colour to frame inputs -----------------------------------------------------
 * What a sensor delivers -- uint16 depth in device units through a distorted lens with its own intrinsics, and the image of a
 * second, colour camera beside it -- becomes what every other entry point reads: per view an undistorted depth map through ONE
 * output pinhole (negative depth, 0 = no measurement), the colour registered to the depth pixels (K17's RGBX, X = 255 where the
 * colour is valid) and a depth map that keeps only the pixels that have a colour (K17's own `depths`).  A background pixel the
 * colour camera cannot see must not take the foreground's colour: the colour camera's z-buffer is splatted with every depth
 * pixel's projected rectangle and a pixel whose depth lies behind the buffer gets no colour.
 * All arithmetic is fp64 with ONE rounding per operation (no contraction, IEEE division; rint rounds half to even), in the order
 * written here, so that tests/ingest_np.py agrees bit for bit on every output and on the z-buffer.
 *
 * distort(x, y; k) with k = (k1, k2, p1, p2, k3), OpenCV's Brown-Conrady order:
 *   r2 = x*x + y*y;  rad = 1 + r2*(k1 + r2*(k2 + r2*k3))
 *   xd = x*rad + ((2*p1)*(x*y) + p2*(r2 + 2*(x*x)));   yd = y*rad + (p1*(r2 + 2*(y*y)) + (2*p2)*(x*y))
 *   If all five coefficients are exactly 0 the function is the identity: it is skipped, not evaluated.
 * ideal(a, b) = ((a - cx)/fx, (b - cy)/fy) with the OUTPUT intrinsics; a, b are pixel coordinates as doubles.
 *
 * A. Decode and rectify, per view and output pixel (i, j) (column, row) of the Hd x Wd output map:
 *   (x, y) = ideal(i, j);  (xd, yd) = distort(x, y; kd);  us = fd[0]*xd + fd[2];  vs = fd[1]*yd + fd[3]      (fd = fx fy cx cy)
 *   (si, sj) = (rint us, rint vs); inside iff 0 <= si <= Wd-1 and 0 <= sj <= Hd-1 (a NaN fails).  Nearest only: depth is never
 *   interpolated across a discontinuity.   raw = raw_depth[sj][si];  z = (double)raw * depth_scale
 *   valid iff inside, raw != 0, z >= z_min and (z_max <= 0 or z <= z_max);   depth_out = valid ? (float)(-z) : 0.0f
 * B. Splat (colour given).  zbuf (n_views x Hc x Wc uint32) is filled with 0xffffffff by the call itself.  For every valid
 *   pixel the three points (a, b) = (i, j), (i - 0.5, j - 0.5), (i + 0.5, j + 0.5), all at the pixel's z:
 *     (x, y) = ideal(a, b);  P = (x*z, y*z, z);  Pc_r = ((T[r][0]*P_0 + T[r][1]*P_1) + T[r][2]*P_2) + T[r][3]   (T = T_dc, 3 x 4)
 *     the pixel is skipped if any of the three Pc_2 is not > 0
 *     (xc, yc) = (Pc_0/Pc_2, Pc_1/Pc_2);  (xcd, ycd) = distort(xc, yc; kc);  u = fc[0]*xcd + fc[2];  v = fc[1]*ycd + fc[3]
 *   With (u1, v1), (u2, v2) of the two corners: skipped unless all four are finite;  a0 = rint(min(u1, u2)), a1 = rint(max(u1, u2)),
 *   b0 = rint(min(v1, v2)), b1 = rint(max(v1, v2));  clipped: a0 = max(a0, 0), a1 = min(a1, Wc-1), b likewise with Hc;  cut:
 *   a1 = min(a1, a0 + max_splat - 1), b1 = min(b1, b0 + max_splat - 1) (a bound on the work per pixel: a condition, not a
 *   tuning knob);  skipped if a0 > a1 or b0 > b1.  key = the bit pattern of (float)Pc_2 of the centre (positive floats order as
 *   unsigned integers);  zbuf[row][col] = min(zbuf[row][col], key) over rows b0..b1, columns a0..a1: a 32-bit integer atomic, so
 *   the buffer does not depend on the order and is the same on every run.
 * C. Gather (colour given), per valid pixel with the centre's (u, v, Pc_2) of B (a centre whose Pc_2 is not > 0 has no colour;
 *   the corners play no part here):
 *   inside iff 0 <= u < Wc-1 and 0 <= v < Hc-1 (a NaN fails: dfh_gn_photometric's visibility rule, so all four taps exist)
 *   occluded iff (double)as_float(zbuf[rint v][rint u]) + occl_tol < (double)(float)Pc_2  (both sides through float32: a pixel
 *   never occludes itself at occl_tol = 0; an untouched entry is a NaN and occludes nothing; occl_tol = +inf: no test)
 *   sample == 1, bilinear: i0 = floor u, j0 = floor v, fu = u - i0, fv = v - j0, per channel with the taps as doubles
 *     c = (1 - fv)*((1 - fu)*c[j0][i0] + fu*c[j0][i0+1]) + fv*((1 - fu)*c[j0+1][i0] + fu*c[j0+1][i0+1]);  byte = (int)rint(c)
 *   sample == 0, nearest: the pixel [rint v][rint u]
 *   color_out = R | G<<8 | B<<16 | 255<<24 where the pixel is valid, inside and not occluded, 0 elsewhere (K17 and K18 ignore X)
 *   color_depth_out (may be NULL) = color_out != 0 ? depth_out : 0.0f
 * At most three launches, all views in each; nothing is copied from or synchronised with the host.  The views' calibration
 * travels as kernel arguments and is left, as a table, behind the z-buffer in the workspace for the launches that follow.
 * zbuf: dfh_rgbd_ingest_workspace_bytes(n_views, Hc, Wc) bytes, 8-byte aligned (0: bad sizes); its first n_views*Hc*Wc dwords
 * are the z-buffer after the call.  raw_color == NULL: only A runs; Hc, Wc, C, the colour side of the views, color_out,
 * color_depth_out and zbuf are not read.
 * DFH_E_BADARG before any HIP call: a null params, raw_depth, views or depth_out; n_views outside 1..16; a null raw_depth[v] or
 * raw_color[v]; Hd or Wd < 2 or Hd*Wd >= 2^31; with colour the same of Hc, Wc, C not 3 or 4, a null color_out or zbuf, a zbuf not
 * 8-byte aligned, a 4-channel image not 4-byte aligned; fx, fy, cx, cy not finite or fx, fy <= 0; any non-finite fd, kd, fc, kc,
 * T_dc; fd[0], fd[1] <= 0; with colour fc[0], fc[1] <= 0; depth_scale not finite or <= 0; a NaN z_min or z_max; occl_tol negative
 * or NaN; max_splat outside 1..16; sample not 0 or 1.
 * dfh_rgbd_ingest_tile: the output tile (rows, columns) per workgroup, for tests that put image sizes on its edges. */
typedef struct dfh_rgbd_view {
    double fd[4], kd[5];          /* raw depth camera: fx fy cx cy; k1 k2 p1 p2 k3 */
    double fc[4], kc[5];          /* colour camera */
    double T_dc[12];              /* row-major 3 x 4, depth camera -> colour camera, in the units of z = raw * depth_scale */
} dfh_rgbd_view;
typedef struct dfh_rgbd_ingest_params {
    int n_views;                  /* 1..16 */
    const void *const *raw_depth; /* HOST array of n_views device pointers, Hd x Wd uint16 row-major */
    const void *const *raw_color; /* HOST array of n_views device pointers, Hc x Wc x C uint8; NULL: no colour */
    int Hd, Wd, Hc, Wc, C;        /* C: 3 | 4 */
    double fx, fy, cx, cy;        /* the output pinhole every depth_out map is resampled to */
    double depth_scale;           /* z = raw * depth_scale; finite, > 0 */
    double z_min, z_max;          /* valid range of z; z_max <= 0: no upper bound */
    double occl_tol;              /* >= 0, in the units of z */
    int max_splat;                /* 1..16 */
    int sample;                   /* 0 nearest | 1 bilinear */
    const dfh_rgbd_view *views;   /* HOST array of n_views records */
} dfh_rgbd_ingest_params;
int dfh_rgbd_ingest(const dfh_rgbd_ingest_params *p, float *depth_out /* n_views x Hd x Wd */, void *color_out /* n_views x Hd x Wd dwords */,
                    float *color_depth_out /* n_views x Hd x Wd, may be NULL */, void *zbuf, void *stream);
size_t dfh_rgbd_ingest_workspace_bytes(int n_views, int Hc, int Wc);
int dfh_rgbd_ingest_tile(int tile_hw[2]);

/* ---- K20  ray cast: depth, normal, colour and hit maps of a TSDF volume seen from up to 16 cameras ---------------------------
 * KinectFusion's surface prediction (no reference counterpart: the reference shows its model only as a mesh).  The volume is only
 * read.  All arithmetic is fp64 with ONE rounding per operation (no contraction, IEEE division and square root), in the order
 * written here; float32 T / w / rgbw values are widened at load and every output is rounded once, at its store, so that
 * tests/raycast_np.py agrees bit for bit.  a ? b : c below is a select: a comparison with a NaN is false.
 *
 * Grid: lo = (x0, 0, 0), hi = (x1 - 1, res_1 - 1, res_2 - 1): the region where a full trilinear cell of the slab exists.  A slab
 * with hi_a < lo_a + 1 on some axis has no cell: every pixel is a miss.
 * S(p), the value at an index-space point p (three doubles), K6v's standard trilinear cell (dfh_gn_associate_volume's axis order):
 *   c_a = floor(p_a);  c_a = c_a >= lo_a ? c_a : lo_a;  c_a = c_a <= hi_a - 1 ? c_a : hi_a - 1;  f_a = p_a - c_a
 *     (the clamp only matters for a p that rounding has put a few ulps outside [lo, hi], which then extrapolates by as much; it
 *     also means that no p whatever, a NaN included, reads outside the slab)
 *   u_ijk = (double)T[c + (i, j, k)];   d_jk.. : dz00 = u001 - u000, dz01 = u011 - u010, dz10 = u101 - u100, dz11 = u111 - u110
 *   e00 = u000 + f_2*dz00, e01 = u010 + f_2*dz01, e10 = u100 + f_2*dz10, e11 = u110 + f_2*dz11
 *   h0 = e00 + f_1*(e01 - e00), h1 = e10 + f_1*(e11 - e10);   t = h0 + f_0*(h1 - h0)
 *   known iff min_weight == 0 (w is not read at all) or every one of the eight corners has (double)w >= min_weight.
 * Per view v and pixel (y, x), X = (double)x, Y = (double)y:
 *  1. ray.  rho_r = (Kinv[r][0]*X + Kinv[r][1]*Y) + Kinv[r][2];  d_r = (wl[r][0]*rho_0 + wl[r][1]*rho_1) + wl[r][2]*rho_2  (wl: the
 *     view's camera -> world 3 x 4, the inverse of lw);  o_a = (wl[a][3] - center_a)/scale + half;  e_a = d_a/scale.  The ray is
 *     parameterised by the depth value z (the third component of K*lpos, what a depth map stores negated): the camera point is
 *     z*rho and the index point i(z)_a = o_a + z*e_a.  L = sqrt((e_0*e_0 + e_1*e_1) + e_2*e_2); a miss unless 0 < L < inf.
 *  2. clip.  zlo = z_near, zhi = z_far; for a = 0, 1, 2: e_a == 0: a miss unless lo_a <= o_a <= hi_a (no division); otherwise
 *     t1 = (lo_a - o_a)/e_a, t2 = (hi_a - o_a)/e_a, tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1, zlo = tn > zlo ? tn : zlo,
 *     zhi = tf < zhi ? tf : zhi.  A miss unless zlo <= zhi.
 *  3. samples.  dz = step/L;  n = floor((zhi - zlo)/dz);  kmax = n < max_steps ? (int)n : max_steps;  sample k = 0..kmax sits at
 *     z_k = zlo + (double)k*dz (a product, never a running sum) and has (known_k, t_k) = S(i(z_k)).
 *  4. walk, k ascending, with a previous sample that starts absent: a sample with known_k, t_k <= 0 and a previous sample is the
 *     crossing: (za, ta) = the previous sample, (zb, tb) = (z_k, t_k), and the walk ends.  Otherwise the previous sample becomes
 *     (z_k, t_k) if known_k and t_k > 0, and absent if not (an unknown sample, a NaN, or a value <= 0 with nothing in front of it:
 *     a ray that starts behind the surface reports nothing until it has seen free space; a - to + transition is never a hit).
 *     No crossing up to kmax: a miss.
 *  5. root.  z* = za + (zb - za)*(ta/(ta - tb));  then `refine` times: (known, t) = S(i(z*)); unknown: stop; t > 0: (za, ta) =
 *     (z*, t), otherwise (zb, tb) = (z*, t); z* recomputed by the same expression.
 *  6. outputs, each (n_views, H, W, ...) and optional (not all NULL), with p = i(z*):
 *     depth  float32: (float)(-z*); 0 on a miss (the maps' convention: it feeds every consumer of a depth map)
 *     hit    float32 x 3: (float)p_a; on a miss the quiet NaN 0x7fc00000 three times
 *     normals float32 x 3, K12's nh convention: for a = 0, 1, 2: g_a = S(p + unit_a) - S(p - unit_a); each of the six points q
 *       must have lo_b <= q_b <= hi_b on all axes and be known, otherwise the normal is missing.  To camera space:
 *       m_c = sg*((wl[0][c]*g_0 + wl[1][c]*g_1) + wl[2][c]*g_2), sg = scale > 0 ? 1 : -1;  l2 = (m_0*m_0 + m_1*m_1) + m_2*m_2;
 *       missing unless 0 < l2 < inf;  nh = m / sqrt(l2) (three divisions);  c = (nh_0*(z* rho_0) + nh_1*(z* rho_1)) + nh_2*(z* rho_2);
 *       c > 0: nh = -nh (the normal faces the camera).  Zeros on a miss or where the normal is missing.
 *     color  uint8 x 4: dfh_sample_colors' rule at p (its own in-grid test, cell, corner order and sums; corners outside the slab
 *       or with wc <= 0 do not count), per channel q = (sum tw*c_a)/S in fp64, byte = q > 0 ? (q >= 255 ? 255 : rint(q)) : 0
 *       (half to even), X = 255; S == 0, outside, or a miss: 0, 0, 0, 0.
 * One march launch serves all views; nothing is copied from or synchronised with the host.  K and lw are not read by the device
 * (the ray needs Kinv and wl only); they travel with the call so that a caller describes a camera as it does everywhere else.
 *
 * Empty-space skipping.  dfh_raycast_table fills one byte per 8 x 8 x 8-cell brick of the slab (brick (b0, b1, b2) = cells
 * [x0 + 8 b0, x0 + 8 b0 + 8) x [8 b1, ..) x [8 b2, ..); ceil((x1 - x0)/8) * ceil(res_1/8) * ceil(res_2/8) bytes, b2 fastest):
 * 0 = dead, 1 = live.  A brick is dead iff every voxel its cells' corners touch, AND the one-voxel ring around them (voxels
 * 8 b_a - 1 .. 8 b_a + 9 per axis, cut at the slab), holds a T with m > 0 and m > M * 2^-30, m and M the least and greatest of those
 * values (a NaN makes the brick live).  With a table the march skips dead bricks without sampling and gives the SAME BITS as
 * without (proof: csrc/dfh_raycast.hip); a table built for another volume state gives wrong images, it is the caller's to keep
 * current.  table == NULL, or the option raycast_skip = 0: the plain march.
 * DFH_E_BADARG before any HIP call: null params or volume; a bad slab; n_views outside 1..16; a null lw or wl; H or W < 1 or
 * H*W >= 2^31; step not finite or <= 0; z_near not finite or < 0; z_far not > z_near (+inf allowed); min_weight negative or NaN;
 * refine outside 0..8; max_steps < 1; scale 0 or not finite; all outputs NULL; color wanted without a colour volume, or with one
 * whose slab is not the volume's; a table of fewer than dfh_raycast_table_bytes bytes.  A slab without a cell: DFH_OK, the
 * outputs are filled with misses, no march is launched.  dfh_raycast_table: a null volume, T or table; a bad slab; an empty
 * slab: DFH_OK, nothing written.  dfh_raycast_table_bytes: 0 for a bad or empty slab. */
typedef struct dfh_raycast_params {
    const dfh_volume *vol;
    const dfh_color_volume *colors;   /* NULL: no colour volume */
    int n_views;                      /* 1..16 */
    int H, W;
    double K[9], Kinv[9];             /* 3x3 row-major */
    const double *lw;                 /* HOST, n_views x 12: world -> camera, as in dfh_depth_views */
    const double *wl;                 /* HOST, n_views x 12: their inverses (camera -> world) */
    double scale, center[3], half;    /* pos = scale*(i - half) + center */
    double z_near, z_far;             /* in the depth maps' units; z_far may be +inf */
    double step;                      /* index-space length between samples, in voxels */
    double min_weight;                /* 0: w is not read */
    int refine;                       /* 0..8 */
    int max_steps;                    /* >= 1; values above 2^30 act as 2^30 */
    const void *table;                /* DEVICE, dfh_raycast_table's; NULL: plain march */
    size_t table_bytes;
    float *depth;                     /* DEVICE outputs, any may be NULL, not all */
    float *normals;
    unsigned char *color;
    float *hit;
} dfh_raycast_params;
size_t dfh_raycast_table_bytes(const dfh_slab *slab);
int dfh_raycast_table(const dfh_volume *vol, void *table, void *stream);
int dfh_raycast(const dfh_raycast_params *p, void *stream);

/* ---- K21  camera tracking: depth pyramid and dense projective point-to-plane ICP of a frame against the model -------------------
 * KinectFusion's pose estimation (no reference counterpart): a frame's depth and normal maps (dfh_depth_prep's) are aligned to
 * the model's predicted maps (dfh_raycast's, or a rendered mesh's), coarse to fine.  Both normal maps share one convention:
 * camera space, facing the camera, zeros for none.  valid(d) is K12's test: d finite and d < 0.
 *
 * dfh_depth_halve: one pyramid step for n_views maps in one launch.  depth: HOST array of n_views device pointers, H x W row-major,
 * DFH_F32 or DFH_F64 (a float64 value is rounded to nearest-even float32 at load); out: DEVICE (n_views, H/2, W/2) float32 (sizes
 * rounded down: an odd last row or column is dropped).  float32 arithmetic, one rounding per operation.  Per output pixel (y, x):
 *   a = D[2y][2x];  a not valid -> 0.  Otherwise sum = 0, n = 0 and, over the taps (2y,2x), (2y,2x+1), (2y+1,2x), (2y+1,2x+1) in
 *   this order, every valid tap e with |e - a| <= (float)max_jump adds sum = sum + e, n = n + 1;  out = sum / (float)n.
 * The level's intrinsics are the caller's: fx/2, fy/2, skew/2, cx' = (cx - 0.5)/2, cy' = (cy - 0.5)/2 (a pixel's coordinate is its
 * integer index).  DFH_E_BADARG before any HIP call: a null depth, depth[v] or out; out equal to a depth[v]; n_views outside
 * 1..16; a dtype other than DFH_F32 / DFH_F64; H or W < 2 or H*W >= 2^31; max_jump not finite or < 0.
 *
 * dfh_icp_track: n_iters Gauss-Newton iterations for all views of ONE pyramid level in one host call; two launches per
 * iteration, nothing is read back in between.  T (DEVICE, n_views x 12 doubles, row-major 3 x 4: live camera -> model camera)
 * is read, updated in place and chained over the iterations.  All arithmetic below is fp64 with ONE rounding per operation (no
 * contraction, IEEE division, square root and rint), float32 map values widened at load; a comparison with a NaN is false.
 * Per view and live pixel (y, x), X = (double)x, Y = (double)y:
 *  1. live validity.  d = live_depth[y][x]; no row unless valid(d).  With live normals l: ll = (l0*l0 + l1*l1) + l2*l2; no row
 *     unless ll > 0.
 *  2. live vertex.  rho_r(X, Y) = (Kinv[r][0]*X + Kinv[r][1]*Y) + Kinv[r][2];  V_r = (-d)*rho_r;
 *     P_r = ((T[r][0]*V_0 + T[r][1]*V_1) + T[r][2]*V_2) + T[r][3].
 *  3. projection.  q_r = (K[r][0]*P_0 + K[r][1]*P_1) + K[r][2]*P_2; no row unless q_2 > 0 and q_2 finite;  ui = rint(q_0/q_2),
 *     vi = rint(q_1/q_2) (half to even); no row unless 0 <= ui <= W-1 and 0 <= vi <= H-1, tested on the doubles.
 *  4. model side.  m = model_depth[vi][ui] must be valid; n = model_normals[vi][ui] with nn = (n0*n0 + n1*n1) + n2*n2 > 0;
 *     M_r = (-m)*rho_r(ui, vi).
 *  5. gates.  e = P - M;  d2 = (e0*e0 + e1*e1) + e2*e2;  max_dist > 0: no row unless d2 <= max_dist*max_dist.  With live normals:
 *     Rl_r = (T[r][0]*l_0 + T[r][1]*l_1) + T[r][2]*l_2;  c = (Rl_0*n_0 + Rl_1*n_1) + Rl_2*n_2;  mm = (Rl_0*Rl_0 + Rl_1*Rl_1) + Rl_2*Rl_2;
 *     no row unless c > 0 and c*c >= (min_cos*min_cos)*(mm*nn)  (K13's form).
 *  6. row.  r = (n_0*e_0 + n_1*e_1) + n_2*e_2;  J = (P x n, n): J0 = P_1*n_2 - P_2*n_1, J1 = P_2*n_0 - P_0*n_2, J2 = P_0*n_1 - P_1*n_0,
 *     J3..5 = n: the derivative of r for a twist (omega, v) applied on the LEFT of T (apply_twist_one's order).
 *     w = huber/|r| if huber > 0 and |r| > huber, else 1.
 *  7. sums per view, 29 values: the 21 upper entries of A = sum w J^T J (row-major, i <= j), the 6 of g = sum w J r, the objective
 *     sum w r^2, the count of rows.  The device forms s = sqrt(w), the products (s*J_i)*(s*J_j), (s*J_i)*(s*r), (s*r)*(s*r) and adds
 *     them on the matrix cores in an order that is fixed (a constant number of workgroups per view, each walking the tiles
 *     b, b + G, ..; their partials added in index order): the same bits on every run and every device, within
 *     (n + 4) 2^-53 sum |w J_i J_j| of the exact sum of n rows.  The count is exact.
 *  8. finish.  count < min_count: no step.  Otherwise D = A with D_ii = A_ii + lm_rel*A_ii, factored D = L L^T column by column,
 *     j = 0..5:  s = D_jj, for k < j ascending s = s - L_jk*L_jk;  a pivot s that is not > 0 and finite refuses the step;
 *     L_jj = sqrt(s);  for i > j: t = D_ij, for k < j ascending t = t - L_ik*L_jk;  L_ij = t / L_jj.
 *     L y = -g: i = 0..5, t = -g_i, for k < i ascending t = t - L_ik*y_k, y_i = t / L_ii.  L^T xi = y: i = 5..0, t = y_i, for
 *     k = i+1..5 ascending t = t - L_ki*xi_k, xi_i = t / L_ii.  ww = (xi_0*xi_0 + xi_1*xi_1) + xi_2*xi_2, vv likewise of xi_3..5;
 *     the step is refused unless ww <= max_rot*max_rot and vv <= max_trans*max_trans (a NaN refuses).
 *     Taken: T <- exp(xi) T.  ww < 1e-8: a = 1 - ww/6, b = 0.5 - ww/24, c = 1/6 - ww/120; otherwise th = sqrt(ww),
 *     a = sin(th)/th, b = (1 - cos(th))/ww, c = (th - sin(th))/(ww*th).  Om = [omega]x, Om2_ij = omega_i*omega_j (- ww on the
 *     diagonal);  R_ij = (I_ij + a*Om_ij) + b*Om2_ij;  Vm_ij = (I_ij + b*Om_ij) + c*Om2_ij;  t_r = (Vm_r0*xi_3 + Vm_r1*xi_4) + Vm_r2*xi_5;
 *     T'[r][c] = (R_r0*T[0][c] + R_r1*T[1][c]) + R_r2*T[2][c], + t_r for c = 3.
 *     A refused step leaves T untouched: the iterations after it see the same maps and the same T and refuse again.
 * Outputs: stats, DEVICE doubles (n_views, n_iters, 40): the 29 sums | status (1 stepped, 0 refused) | xi (6, zeros when refused) |
 * 4 zeros.  rows, optional DEVICE doubles (n_views, H, W, 8): J0..5 | r | w of the FIRST iteration (the one that reads the
 * caller's T), all zero where there is no row.  scratch: DEVICE, dfh_icp_track_bytes(n_views) bytes, no initial state.
 * live_depth (V,H,W), model_depth (V,H,W), model_normals (V,H,W,3), live_normals (V,H,W,3) or NULL (no normal gate, no ll test):
 * DEVICE float32, view-major, contiguous, only read.  n_iters == 0: DFH_OK, nothing launched.
 * DFH_E_BADARG before any HIP call: null params; n_views outside 1..16; H or W < 1 or H*W >= 2^31; a null live_depth,
 * model_depth, model_normals, T or scratch, a null stats with n_iters > 0; a K or Kinv entry that is not finite; max_dist, huber or lm_rel negative or
 * not finite; min_cos outside [0, 1]; n_iters outside 0..64; min_count < 6; max_rot or max_trans not > 0; a scratch smaller
 * than dfh_icp_track_bytes (which is 0 for n_views outside 1..16). */
typedef struct dfh_icp_track_params {
    int n_views;                      /* 1..16 */
    int H, W;
    const float *live_depth;          /* DEVICE (V, H, W) */
    const float *live_normals;        /* DEVICE (V, H, W, 3) or NULL */
    const float *model_depth;         /* DEVICE (V, H, W) */
    const float *model_normals;       /* DEVICE (V, H, W, 3) */
    double K[9], Kinv[9];             /* 3x3 row-major, of this level */
    double *T;                        /* DEVICE, V x 12, in and out */
    double max_dist;                  /* 0: no distance gate */
    double min_cos;                   /* 0..1 */
    double huber;                     /* 0: no robust weight */
    double lm_rel;
    int n_iters;                      /* 0..64 */
    int min_count;                    /* >= 6 */
    double max_rot, max_trans;        /* largest |omega| and |v| of one step */
    double *stats;                    /* DEVICE (V, n_iters, 40) */
    double *rows;                     /* DEVICE (V, H, W, 8) or NULL */
    void *scratch;                    /* DEVICE */
    size_t scratch_bytes;
} dfh_icp_track_params;
int dfh_depth_halve(const void *const *depth, int n_views, int depth_dtype, int H, int W, double max_jump, float *out, void *stream);
size_t dfh_icp_track_bytes(int n_views);
int dfh_icp_track(const dfh_icp_track_params *p, void *stream);

/* ---- K22  mesh -> signed distance: exact point-to-mesh distance, closest point, face and pseudonormal sign --------------------
 * No reference counterpart (the reference reads `.dist` files made by an external tool).  Vertices are fp64; all arithmetic is
 * fp64 with ONE rounding per operation; dot(u, v) = (u0*v0 + u1*v1) + u2*v2; a comparison with a NaN is false.
 *
 * Closest point of P on one face (A, B, C), Ericson's walk.  ab = B - A, ac = C - A, ap = P - A, bp = P - B, cp = P - C;
 *   d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
 *   vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4.  The first region that holds wins (feature id in brackets):
 *   [0] d1 <= 0 and d2 <= 0: Q = A.            [1] d3 >= 0 and d4 <= d3: Q = B.
 *   [3] vc <= 0, d1 >= 0, d3 <= 0: Q = A + (d1/(d1 - d3))*ab.            [2] d6 >= 0 and d5 <= d6: Q = C.
 *   [4] vb <= 0, d2 >= 0, d6 <= 0: Q = A + (d2/(d2 - d6))*ac.
 *   [5] va <= 0, d4 - d3 >= 0, d5 - d6 >= 0: Q = B + ((d4 - d3)/((d4 - d3) + (d5 - d6)))*(C - B).
 *   [6] otherwise: den = 1/((va + vb) + vc), Q = (A + (vb*den)*ab) + (vc*den)*ac.
 *   D2 = dot(P - Q, P - Q).
 * Winner: the face with the smallest D2, the lowest index on ties, over the faces with keep[f] != 0 (the caller clears keep for
 * the faces whose ab x ac is the exact zero vector).  A minimum over a set: no search order can change it.
 * Sign: N = face_normals[f] (feature 6), edge_normals[f][feature - 3] (3..5) or vertex_normals[faces[f][feature]] (0..2), the
 * caller's angle-weighted pseudonormal tables; the value is negative iff dot(P - Q, N)*orientation < 0 and D2 != 0; D2 == 0 gives
 * +0.0.  Known iff D2 <= band*band (band = +inf: always).  Known: value = +-sqrt(D2) rounded once to the output type, closest = Q
 * rounded to float32, face = the winner.  Far: face = -1, closest = NaN, value = +band (points).
 * Grid vertex (i, j, k) is at origin_a + (double)idx_a*spacing_a; outputs are (X, Y, Z) row-major, z fastest.  Far fill (grids,
 * finite band): three sweeps, along z, then y, then x.  Along each line an undecided (far) vertex takes the sign of the preceding
 * decided vertex of the line, the vertices before the first decided one take that one's sign, a line with nothing decided is
 * left to the next sweep; whatever is left after x is +.  A far vertex's value is +-band.
 *
 * dfh_mesh_sdf_plan (HOST arrays, no device work): checks the mesh and lays out the cell table -- the box of the kept faces, the
 * cell edge (cell == 0: twice the mean face extent; never below extent/127, so that an axis has at most 128 cells), the entry
 * count.  dfh_mesh_sdf_build fills the table on the device (count -> scan -> fill).  The queries then walk it shell by shell
 * (csrc/dfh_mesh_sdf.hip has the proof of the stopping rule).  dfh_mesh_sdf_chunk: faces staged in LDS per evaluation pass.
 * DFH_E_BADARG before any device work -- plan: a null array, n_faces == 0, a vertex index outside [0, n_verts), a vertex
 * coordinate that is not finite, no kept face, cell negative or not finite, 2^31 entries or more; build and the queries: a null
 * mesh or mesh array, a layout that is not plan's for these counts, a table smaller than layout.bytes; the queries: band not
 * > 0 (NaN included), orientation not +-1, null points / sdist with n > 0, a null value, a bad dtype, a shape entry < 1, 2^31
 * vertices or more, an origin that is not finite, a spacing not finite or <= 0, a finite band below max(spacing) or without
 * the status workspace. */
typedef struct dfh_mesh_sdf_layout {
    double lo[3], hi[3];              /* box of the kept faces = the table's box */
    double cell;                      /* cell edge in use */
    double maxabs;                    /* largest |vertex coordinate| */
    int dims[3];                      /* cells per axis, 1..128 */
    long n_verts, n_faces, n_entries;
    size_t bytes;                     /* of the device table */
} dfh_mesh_sdf_layout;
typedef struct dfh_mesh_sdf {
    const double *verts;              /* DEVICE (n_verts, 3) */
    const int *faces;                 /* DEVICE (n_faces, 3) */
    const unsigned char *keep;        /* DEVICE (n_faces) */
    const double *face_normals;       /* DEVICE (n_faces, 3) */
    const double *edge_normals;       /* DEVICE (n_faces, 3, 3): local edges AB, AC, BC */
    const double *vertex_normals;     /* DEVICE (n_verts, 3) */
    long n_verts, n_faces;
    void *table;                      /* DEVICE, layout.bytes */
    size_t table_bytes;
    dfh_mesh_sdf_layout layout;       /* dfh_mesh_sdf_plan's */
} dfh_mesh_sdf;
typedef struct dfh_mesh_sdf_grid_params {
    double origin[3], spacing[3];
    int shape[3];
    double band;                      /* > 0 or +inf */
    int orientation;                  /* +1: faces wind outward */
    int dtype;                        /* DFH_F32 / DFH_F64 of value */
    void *value;                      /* DEVICE (X, Y, Z) */
    signed char *status;              /* DEVICE (X, Y, Z) workspace, needed with a finite band */
    float *closest;                   /* DEVICE (X, Y, Z, 3) or NULL */
    int *face;                        /* DEVICE (X, Y, Z) or NULL */
} dfh_mesh_sdf_grid_params;
int dfh_mesh_sdf_chunk(void);
int dfh_mesh_sdf_plan(const double *verts, long n_verts, const int *faces, const unsigned char *keep, long n_faces, double cell,
                      dfh_mesh_sdf_layout *out);
int dfh_mesh_sdf_build(const dfh_mesh_sdf *m, void *stream);
int dfh_mesh_sdf_points(const dfh_mesh_sdf *m, const double *points, long n, double band, int orientation, double *sdist,
                        float *closest, int *face, void *stream);
int dfh_mesh_sdf_grid(const dfh_mesh_sdf *m, const dfh_mesh_sdf_grid_params *g, void *stream);

/* ---- K23  mesh connected components: label, measure, compact --------------------------------------------------------------------
 * No reference counterpart.  verts: DEVICE (V, 3) float32 or float64 (dtype DFH_F32 / DFH_F64; float32 is widened, exactly, before
 * anything is computed); faces: DEVICE (F, 3) int32.  Every output is a function of the mesh alone: the order in which the
 * kernels' integer atomics land shows in none of them.
 *
 * Connectivity.  Two vertices are connected when some face names both; components are the classes of the transitive closure; a
 *   face belongs to the component of its vertices.  A degenerate face (a == b) still connects what it names, duplicate faces
 *   count once each, a vertex that no face names is a component of its own with 0 faces.
 * Labels.  root[v] = the lowest vertex index of v's component.  Component ids are 0 .. C-1 in ascending order of root:
 *   vert_comp[v] = the number of roots below root[v], face_comp[f] = vert_comp[faces[f][0]].
 * Table, per component c.  comp_root[c]; n_verts[c]; n_faces[c]; the box; the area.
 *   Box.  key(x) for a double x that is not a NaN: its 64 bits b as an unsigned integer, ~b if the sign bit is set, else
 *   b | 2^63 (so key(x) < key(y) <=> x < y, and -0.0 lies below +0.0).  bbox_min[c][a] = the coordinate with the smallest key
 *   over the component's vertices, bbox_max[c][a] the one with the largest; if any of those coordinates is a NaN the entry is
 *   the NaN with bits 0x7ff8000000000000.
 *   Area of a face (A, B, C), fp64, one rounding per operation, no contraction: e1 = B - A, e2 = C - A; cx = e1y*e2z - e1z*e2y,
 *   cy = e1z*e2x - e1x*e2z, cz = e1x*e2y - e1y*e2x (two rounded products and one subtraction each);
 *   s = (cx*cx + cy*cy) + cz*cz; area = 0.5*sqrt(s).
 *   Area of a component, the order of the additions.  Chunk j = the faces [256 j, 256 j + 256).  P(j, c) = the areas of chunk
 *   j's faces of component c, added in ascending face index starting from the first.  area[c] = the P(j, c) of the chunks that
 *   hold a face of c, added in ascending j starting from the first; +0.0 for a component without faces.  No float atomics.
 *   Coordinates that are not finite reach the box and the area of their own component only: labels and counts read no coordinate.
 * Compaction.  keep: DEVICE uint8 per component.  A face survives when keep[face_comp[f]] != 0.  A vertex survives when
 *   keep[vert_comp[v]] != 0 and, with drop_unreferenced = 1, some surviving face names it.  kept_vert_idx: the surviving
 *   vertices' old indices, ascending (V entries of room); vert_map[v] = the new index, -1 for a dropped vertex; faces_out: the
 *   surviving faces in their original order, indices through vert_map (F x 3 of room).  counts_out: HOST long[2] = (vertices,
 *   faces) that survive.  Per-vertex attributes are gathered by the caller with kept_vert_idx.
 *
 * workspace: dfh_mesh_components_workspace_bytes(V, F) bytes of device memory, 8-byte aligned, the same size for the three
 * calls (0 for counts the calls refuse); its contents carry nothing from one call to the next.
 * dfh_mesh_components and dfh_mesh_compact do not only enqueue: each queues its kernels on `stream`, synchronises `stream`, and
 * has written n_components / counts_out (HOST pointers) when it returns -- the caller sizes what follows from them.  Like
 * dfh_radius_sample they cannot be captured into a graph.  dfh_mesh_component_table only enqueues.
 * Bad indices.  A face index outside [0, V) touches no memory: the face joins nothing, face_comp[f] = -1, a device flag is
 * raised and dfh_mesh_components returns DFH_E_BADARG once it has synchronised (root / vert_comp then describe the mesh without
 * those faces).  dfh_mesh_compact does the same for a face index outside [0, V) or a component id outside [0, C); the table
 * call skips such faces and vertices.
 * V == 0 or F == 0 are valid and launch nothing they do not need; V == 0 and F == 0 launches nothing.  DFH_E_BADARG before any
 * HIP call: V or F negative or >= 2^31; C < 0 or C > V; a null n_components / counts_out; a null array of a non-zero count
 * (keep with C > 0); a dtype other than DFH_F32 / DFH_F64; drop_unreferenced other than 0 / 1; a null workspace, one that is not
 * 8-byte aligned or one smaller than dfh_mesh_components_workspace_bytes(V, F). */
size_t dfh_mesh_components_workspace_bytes(long n_verts, long n_faces);
int dfh_mesh_components(const int *faces, long n_verts, long n_faces, int *root, int *vert_comp, int *face_comp,
                        long *n_components, void *workspace, size_t workspace_bytes, void *stream);
int dfh_mesh_component_table(const void *verts, int dtype, long n_verts, const int *faces, long n_faces, const int *root,
                             const int *vert_comp, const int *face_comp, long n_components, int *comp_root, int *comp_n_verts,
                             int *comp_n_faces, double *bbox_min, double *bbox_max, double *area, void *workspace,
                             size_t workspace_bytes, void *stream);
int dfh_mesh_compact(const int *faces, long n_verts, long n_faces, const int *vert_comp, const int *face_comp,
                     const unsigned char *keep, long n_components, int drop_unreferenced, int *kept_vert_idx, int *vert_map,
                     int *faces_out, long *counts_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- K24  mesh simplification: vertex clustering with quadric error metrics --------------------------------------------------------
 * No reference counterpart.  verts: DEVICE (V, 3) float32 or float64 (dtype DFH_F32 / DFH_F64; float32 is widened, exactly, before
 * anything is computed); faces: DEVICE (F, 3) int32; cell > 0; origin: HOST double[3]; mode DFH_SIMPLIFY_QUADRIC / _MEAN; reg >= 0.
 * All arithmetic is fp64, one rounding per operation, no contraction; every sum starts at 0.0 and adds one term after the other
 * in the stated order.  Every output is a function of the mesh and the parameters alone: the order in which the kernels'
 * integer atomics land shows in none of them, and there is no float atomic.
 *
 * Cells.  c_a = floor((p_a - origin_a) / cell) per axis (one subtraction, one division).  key = c0 2^42 + c1 2^21 + c2.  The
 *   centre of the cell is ctr_a = origin_a + (c_a + 0.5) * cell.
 * Clusters.  A cluster is the set of vertices with one key, referenced by a face or not.  Cluster ids are 0 .. C-1 in ascending
 *   order of the cluster's lowest vertex index; vert_cluster[v] is v's.  Its members in ascending vertex index are
 *   order[cluster_start[c] .. + cluster_count[c]), order being the stable ascending sort of the keys that the caller supplies.
 * Mean.  S = the sum of (p - ctr) over the members in ascending vertex index, per axis; m = S / double(count).
 * Vertex quadric.  For face f = (a, b, c): e1 = p_b - p_a, e2 = p_c - p_a, n = e1 x e2 with n0 = e1y*e2z - e1z*e2y,
 *   n1 = e1z*e2x - e1x*e2z, n2 = e1x*e2y - e1y*e2x (two rounded products and a subtraction each).  For the corner of f at vertex
 *   v: q = p_a - ctr(cluster of v), d = -((n0*q0 + n1*q1) + n2*q2), and the ten numbers (n0n0, n0n1, n0n2, n1n1, n1n2, n2n2,
 *   d n0, d n1, d n2, d d).  Q_v = their sums over the (face, corner) entries that name v, in ascending face then corner order
 *   (corner_order[corner_begin[v] .. corner_end[v]) holds those entries as 3 f + corner: the stable ascending sort of the 3F
 *   corner entries by the vertex they name, supplied by the caller).  The weight of a face is its area squared times four: no
 *   square root, no division.
 * Cluster quadric.  Q_C = the sum of Q_v over the members in ascending vertex index; A = its first six numbers as a symmetric
 *   3 x 3 matrix (A00 A01 A02 A11 A12 A22), b = the next three.
 * Representative x, relative to ctr.  mode MEAN: x = m.  mode QUADRIC: t = (A00 + A11) + A22; if !(t > 0), x = m.  Otherwise
 *   lam = reg * t, M = A + lam I, r_a = lam * m_a - b_a, and M x = r is solved by LDL^T in this order:
 *     d0 = M00;  l10 = M10 / d0;  l20 = M20 / d0;  d1 = M11 - l10*M10;  t21 = M21 - l20*M10;  l21 = t21 / d1;
 *     d2 = (M22 - l20*M20) - l21*t21;  y0 = r0;  y1 = r1 - l10*y0;  y2 = (r2 - l20*y0) - l21*y1;
 *     x2 = y2 / d2;  x1 = y1 / d1 - l21*x2;  x0 = (y0 / d0 - l10*x1) - l20*x2.
 *   If a pivot d0, d1, d2 is !(> 0) (tested as it is formed, before it divides), or unless every |x_a| <= cell / 2, x = m and
 *   the cluster counts as fallen back.  n_fallback: DEVICE int, the clusters that fell back (0 in mode MEAN).
 *   verts_out[c][a] = ctr_a + x_a, cast to the dtype of verts ((C, 3) of room).
 * Attributes.  attr: DEVICE (V, width) of dtype; out[c][k] = the fp64 sum of attr[v][k] over the members in ascending vertex
 *   index, divided by double(count), cast to dtype.
 * Faces.  A face is remapped through vert_cluster; it is dropped if two of its corners are equal; among the faces with the same
 *   unordered triple the one with the lowest index survives.  With drop_unreferenced = 1 a cluster survives when a surviving face
 *   names it, otherwise every cluster does.  cluster_map[c] = the survivors in front of c, -1 for a dropped cluster;
 *   kept_cluster_idx = the survivors' ids, ascending (C of room); faces_out = the surviving faces in their order, corner order
 *   kept, ids through cluster_map (F x 3 of room); face_idx = their old indices, ascending (F of room); vert_map[v] =
 *   cluster_map[vert_cluster[v]].  counts_out: HOST long[2] = (clusters, faces) that survive.  The result is not guaranteed
 *   manifold or consistently oriented where sheets thinner than a cell collapse.
 *
 * The calls, in order: _keys (keys per vertex; the caller sorts them, and the flattened faces, stably), _group (clusters and
 * corner lists from the two sorted arrays), _clusters (positions), _attr (once per attribute), _faces.
 * workspace: dfh_mesh_simplify_workspace_bytes(V, F) bytes of device memory, 8-byte aligned, the same size for the four calls
 * that take one (0 for counts the calls refuse); its contents carry nothing from one call to the next.
 * _keys, _group and _faces do not only enqueue: each queues its kernels on `stream`, synchronises `stream`, and has written
 * n_clusters / counts_out (HOST pointers) when it returns.  Like dfh_mesh_components they cannot be captured into a graph.
 * _clusters and _attr only enqueue.
 * Refused on the device.  _keys raises a device flag and returns DFH_E_BADARG once it has synchronised for a coordinate that is
 * not finite, a c_a outside [0, 2^21) or a face index outside [0, V) (such a vertex's key is -1; nothing is addressed through a
 * bad index).  Every later call range-checks each index it addresses memory with -- a face's corners, the entries of order and
 * corner_order, cluster ids, segments -- skips what fails, and _group / _faces return DFH_E_BADARG for it.
 * V == 0 or F == 0 are valid and launch nothing they do not need.  DFH_E_BADARG before any HIP call: V negative or >= 2^31; F
 * negative or above (2^31 - 1) / 3; a width negative or >= 2^31; C < 0 or C > V; faces without vertices or clusters; a cell
 * that is not finite or not above 0; an origin or reg that is not finite, a negative reg; a mode or dtype that is not one of
 * the two; drop_unreferenced other than 0 / 1; a null origin, n_clusters, n_fallback or counts_out; a null array of a non-zero
 * count; a null workspace, one that is not 8-byte aligned or one smaller than dfh_mesh_simplify_workspace_bytes(V, F). */
#define DFH_SIMPLIFY_QUADRIC 0
#define DFH_SIMPLIFY_MEAN 1
size_t dfh_mesh_simplify_workspace_bytes(long n_verts, long n_faces);
int dfh_mesh_simplify_keys(const void *verts, int dtype, long n_verts, const int *faces, long n_faces, double cell,
                           const double *origin, long long *keys, void *workspace, size_t workspace_bytes, void *stream);
int dfh_mesh_simplify_group(const long long *sorted_keys, const long long *order, long n_verts, const int *sorted_corner_vert,
                            long n_faces, int *vert_cluster, int *cluster_start, int *cluster_count, int *corner_begin,
                            int *corner_end, long *n_clusters, void *workspace, size_t workspace_bytes, void *stream);
int dfh_mesh_simplify_clusters(const void *verts, int dtype, long n_verts, const int *faces, long n_faces, double cell,
                               const double *origin, int mode, double reg, const long long *keys, const long long *order,
                               const long long *corner_order, const int *corner_begin, const int *corner_end,
                               const int *cluster_start, const int *cluster_count, long n_clusters, void *verts_out,
                               int *n_fallback, void *workspace, size_t workspace_bytes, void *stream);
int dfh_mesh_simplify_attr(const void *attr, int dtype, long n_verts, long width, const long long *order, const int *cluster_start,
                           const int *cluster_count, long n_clusters, void *out, void *stream);
int dfh_mesh_simplify_faces(const int *faces, long n_verts, long n_faces, const int *vert_cluster, long n_clusters,
                            int drop_unreferenced, int *faces_out, int *face_idx, int *cluster_map, int *kept_cluster_idx,
                            int *vert_map, long *counts_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- K25  mesh smoothing (Taubin's lambda|mu filter over a fixed Laplacian) and area-weighted vertex normals ----------------------
 * No reference counterpart.  verts: DEVICE (V, 3) float32 or float64 (dtype DFH_F32 / DFH_F64; float32 is widened, exactly, before
 * anything is computed); faces: DEVICE (F, 3) int32.  All arithmetic is fp64, one rounding per operation, no contraction; every
 * sum starts at 0.0 and adds one term after the other in the stated order.  Every output is a function of the mesh and the
 * parameters alone: there is no float atomic, and the only integer atomic is the error flag.
 *
 * Lists.  sorted_corner_vert (3F int32) and corner_order (3F int64) are the values and the indices of the stable ascending sort
 *   of the 3F corner entries faces[f][c] (entry 3 f + c) by the vertex they name, supplied by the caller (K24's grouping).
 *   Sorted entry i, naming corner c of face f and so vertex v = f[c], has the neighbour pair a = f[(c + 1) % 3], b = f[(c + 2) % 3].
 *   The list of v is the sorted entries [corner_begin[v], corner_end[v]): ascending face, then corner.  A vertex no face names
 *   has an empty list.  A face may name a vertex twice; its entries are listed like any other (a or b is then v itself).
 * Boundary flag.  Vertex v is flagged when, for some u != v, the number of entries equal to u among the 2 (end - begin) neighbour
 *   entries of v is not 2: an open edge (1), a non-manifold edge (3 or more), a repeated face (4).  A vertex with an empty list
 *   is not flagged.  boundary_out: DEVICE V bytes, 0 / 1, or null.
 * Weights.  DFH_SMOOTH_UNIFORM: w_a = w_b = 1 for every entry, and W_v = double(2 (end - begin)), exact.  DFH_SMOOTH_COTANGENT,
 *   from the positions given to _prepare, per entry: e1 = p_a - p_v, e2 = p_b - p_v, n0 = e1y*e2z - e1z*e2y, n1 = e1z*e2x - e1x*e2z,
 *   n2 = e1x*e2y - e1y*e2x, A2 = sqrt((n0*n0 + n1*n1) + n2*n2);  with d = p_v - p_b, g = p_a - p_b:
 *   q_a = ((d0*g0 + d1*g1) + d2*g2) / A2, w_a = q_a if q_a > 0, otherwise 0;  with d = p_v - p_a, g = p_b - p_a: q_b, w_b alike;
 *   w_a = w_b = 0 when !(A2 > 0).  w_a is the cotangent of the face's angle at b, the one opposite the edge (v, a).  A negative
 *   cotangent is clamped to 0 (an obtuse angle would make the operator pull away from a neighbour).  W_v = the sum over the
 *   list, in its order, W += w_a then W += w_b.  The weights are NOT recomputed between passes: the operator is fixed, the
 *   filter linear.
 * Pass.  For a value row x (V, width), width 1 .. 4, with a factor: acc_k = 0.0; for every entry of v's list in order,
 *   acc_k += w_a * (x_a,k - x_v,k), then acc_k += w_b * (x_b,k - x_v,k) (uniform: the product with 1 is the difference itself);
 *   x'_v,k = x_v,k + factor * (acc_k / W_v).  x'_v = x_v where !(W_v > 0) and, with DFH_SMOOTH_FIXED, for a flagged vertex.
 *   Every vertex of a pass reads the values of the pass before (two buffers).
 * Run.  x is widened to fp64; iters times: a pass with factor lam, then a pass with factor mu (skipped when mu == 0.0); the
 *   result is cast to dtype, once.  iters = 0 returns x's bits.  out may be x.  layout DFH_SMOOTH_ROWS / _PLANES chooses how the
 *   fp64 values lie in the workspace between passes (rows of four doubles, or one plane a column); the result's bits do not
 *   depend on it.
 * Vertex normals.  s = the sum over v's list, in order, of (e1y*e2z - e1z*e2y, e1z*e2x - e1x*e2z, e1x*e2y - e1y*e2x) with
 *   e1 = p_a - p_v, e2 = p_b - p_v, taken from the verts given to THIS call (area weighting); m = sign * s;
 *   len = sqrt((m0*m0 + m1*m1) + m2*m2); normals[v] = m / len cast to dtype, or 0 where !(len > 0).  No angle weighting is
 *   offered: it needs acos, whose bits the device and a host restatement do not share.
 *
 * workspace: dfh_mesh_smooth_workspace_bytes(V, F) bytes of device memory, 32-byte aligned, a function of (V, F) alone (0 for
 *   counts the calls refuse).  _prepare writes the lists, the flags and the weights into it; _run and _vertex_normals read them
 *   from the SAME workspace, which the caller keeps for as long as it uses the mesh.  A workspace that was not prepared, or was
 *   prepared with other weights than _run is given, yields undefined values but addresses nothing outside itself and the V rows.
 * _prepare does not only enqueue: it queues its kernels on `stream`, synchronises `stream` once and reads the flag.  _run and
 *   _vertex_normals only enqueue: all passes of a call in one host call, no synchronisation.
 * Refused on the device: _prepare returns DFH_E_BADARG once it has synchronised for a coordinate that is not finite, a face index
 *   outside [0, V), or lists that are not the sort of the faces (nothing is addressed through a bad index).
 * V == 0 or F == 0 are valid and launch nothing they do not need.  DFH_E_BADARG before any HIP call: V negative or >= 2^31; F
 *   negative or above (2^31 - 1) / 3 (3F must fit an int); faces without vertices; width outside 1 .. 4; iters < 0; lam, mu or
 *   sign not finite; a dtype, weights, boundary or layout that is not one of the two; a null array of a non-zero count; a null
 *   workspace, one that is not 32-byte aligned or one smaller than dfh_mesh_smooth_workspace_bytes(V, F). */
#define DFH_SMOOTH_UNIFORM 0
#define DFH_SMOOTH_COTANGENT 1
#define DFH_SMOOTH_FIXED 0
#define DFH_SMOOTH_FREE 1
#define DFH_SMOOTH_ROWS 0
#define DFH_SMOOTH_PLANES 1
size_t dfh_mesh_smooth_workspace_bytes(long n_verts, long n_faces);
int dfh_mesh_smooth_prepare(const void *verts, int dtype, long n_verts, const int *faces, long n_faces,
                            const int *sorted_corner_vert, const long long *corner_order, int weights,
                            unsigned char *boundary_out, void *workspace, size_t workspace_bytes, void *stream);
int dfh_mesh_smooth_run(const void *x, int dtype, long n_verts, long n_faces, long width, int weights, int boundary, int layout,
                        int iters, double lam, double mu, void *out, void *workspace, size_t workspace_bytes, void *stream);
int dfh_mesh_vertex_normals(const void *verts, int dtype, long n_verts, long n_faces, double sign, void *normals, void *workspace,
                            size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DFUSION_HIP_H */
