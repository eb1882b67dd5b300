// K1w  depth maps -> canonical TSDF through the warp field (dfh_integrate_depth_dqb): DynamicFusion's surface fusion.
//
// Every canonical voxel is warped into the live frame by K3's chain (Fusion.warp, reference core/fusion.py:502-551: k nearest
// nodes, Gaussian blend, double dqb_warp), the warped position is projected into each depth map by K1's chain
// (FusionDM.fuseDepths, core/fusion_dm.py:191-203, with the voxel index replaced by the warped position) and the projective
// signed distance is averaged into the voxel: no live volume, no second trilinear resampling.
//
// One voxel per lane.  The searching modes run K3's 4 x 4 x 16 bricks (block_knn stages a brick's candidate nodes through
// LDS), the stored-index mode runs its threads along z.  T and w are read once, updated view by view in registers -- rounded
// to the volume's dtype after every view, so V views in one call are V one-view calls bit for bit -- and written once, and
// only where a view updated them.  Everything is the exact fp64 chain (the library is built with -ffp-contract=off); there
// is no float32 fast path here.
//
// The search, the blend weights and the blended double warp are the functions K3's exact kernel calls (dfh_dqb_front.h).
// Two pieces are restated here because the originals are welded to their kernels:
//   * the voxel decode and the stored-index load / store: the body of fuse_volume_dqb_kernel (dfh_fuse_volume.hip), modes
//     0 / 1 / 2 -- lifting it into a function changed that kernel's register allocation;
//   * the projection chain: exact_voxel (dfh_integrate.hip), which reads a 500-byte per-view IntegrateParams block that
//     sixteen views cannot pass by value and takes an integer voxel index.
#include "dfh_dqb_front.h"

namespace dfh {

void dqb_forget_weights(const void *workspace);        // dfh_fuse_volume.hip

constexpr int kWarpedMaxViews = 16;

struct WarpedView {
    double lw[12];              // 3x4 row-major extrinsic
    const void *depth;          // H x W map of the call's depth dtype
};

// 16 x 104 B + K, Kinv and the index -> world map: 1.9 KB by value in the kernel-argument segment, read through scalar loads
struct WarpedViews {
    Mat3 K, Kinv;
    double scale, cx, cy, cz, half;
    int H, W, n, weight_mode;
    WarpedView v[kWarpedMaxViews];
};

// exact_voxel of dfh_integrate.hip (fusion_dm.py:191-203, its operation order) at a double position q instead of an integer
// voxel index: false = this view does not update the voxel; sd_out = the signed distance where it does.
template <typename DepthT, bool PINHOLE>
__device__ __forceinline__ bool warped_view_sd(const WarpedViews &vw, const WarpedView &view, const D3 &q, double tdist,
                                               double &sd_out) {
    const double *lw = view.lw;
    const double px = vw.scale * (q.x - vw.half) + vw.cx;          // :191
    const double py = vw.scale * (q.y - vw.half) + vw.cy;
    const double pz = vw.scale * (q.z - vw.half) + vw.cz;
    const double l0 = ((lw[0] * px + lw[1] * py) + lw[2] * pz) + lw[3];     // :193
    const double l1 = ((lw[4] * px + lw[5] * py) + lw[6] * pz) + lw[7];
    const double l2 = ((lw[8] * px + lw[9] * py) + lw[10] * pz) + lw[11];
    double p0, p1, p2;
    if (PINHOLE) {          // K = [[fx,0,cx],[0,fy,cy],[0,0,1]]: the dropped terms are exact zeros
        p0 = vw.K.m[0] * l0 + vw.K.m[2] * l2;
        p1 = vw.K.m[4] * l1 + vw.K.m[5] * l2;
        p2 = l2;
    } else {
        p0 = (vw.K.m[0] * l0 + vw.K.m[1] * l1) + vw.K.m[2] * l2;
        p1 = (vw.K.m[3] * l0 + vw.K.m[4] * l1) + vw.K.m[5] * l2;
        p2 = (vw.K.m[6] * l0 + vw.K.m[7] * l1) + vw.K.m[8] * l2;
    }
    if (!(p2 != 0.0)) return false;                                 // util.py:318
    const double u = p0 / p2;
    const double v = p1 / p2;
    // (a warped position that is not finite fails here: every comparison with a NaN is false)
    if (!((u >= 0.0) && (u < (double)(vw.W - 1)) && (v >= 0.0) && (v < (double)(vw.H - 1)))) return false;  // :195
    const int ui = (int)rint(u);                                    // Python round(): half to even (:196)
    const int vi = (int)rint(v);
    const double zd = -1.0 * (double)static_cast<const DepthT *>(view.depth)[(size_t)vi * vw.W + ui];
    if (!(zd > 0.0)) return false;                                  // :197
    double cz;
    if (PINHOLE) {
        cz = zd;                                                    // Kinv row 2 == [0,0,1]
        // ... unless z u or z v overflows: the reference multiplies them with Kinv's zeros, 0 * inf = NaN, and a NaN sd
        // updates nothing (exact_voxel's rule)
        if (!((zd * u < __builtin_huge_val()) & (zd * v < __builtin_huge_val()))) return false;
    } else {
        cz = (vw.Kinv.m[6] * (zd * u) + vw.Kinv.m[7] * (zd * v)) + vw.Kinv.m[8] * (zd * 1.0);
    }
    const double sd = cz - l2;                                      // :201
    sd_out = sd;
    return sd > -1.0 * tdist;                                       // :203
}

// MODE 0: search the brick's candidates; 1: search and store per voxel the k node indices; 2: load the stored indices.
// The blend weights are recomputed from the node positions in every mode: the weight region of a level-2 workspace is
// K3's alone.
template <typename VolT, typename DepthT, int KS, int MODE, bool PINHOLE>
__global__ __launch_bounds__(256) void integrate_depth_dqb_kernel(VolT *__restrict__ tsdf, VolT *__restrict__ tsdf_w,
                                                                   const double *__restrict__ node_pos,
                                                                   const double *__restrict__ node_dq,
                                                                   const double *__restrict__ node_w,
                                                                   const int *__restrict__ cand,
                                                                   unsigned short *__restrict__ knn_cache, const DqbParams p,
                                                                   const WarpedViews vw) {
    // ---- which voxel, which nodes: fuse_volume_dqb_kernel's decode and index cache (dfh_fuse_volume.hip), modes 0 / 1 / 2
    const size_t nvox = (size_t)p.nx * p.Y * p.Z;
    const long brick = blockIdx.x;
    int xl, y, z;
    bool inb;
    if (MODE >= 2) {            // no search, no bricks: threads run along z (whole 128-B lines of every per-voxel array)
        const size_t lin = (size_t)blockIdx.x * 256 + threadIdx.x;
        inb = lin < nvox;
        z = (int)(lin % (size_t)p.Z);
        y = (int)((lin / (size_t)p.Z) % (size_t)p.Y);
        xl = (int)(lin / ((size_t)p.Z * p.Y));
    } else {
        const int bz = (int)(brick % p.nbz);
        const int by = (int)((brick / p.nbz) % p.nby);
        const int bx = (int)(brick / ((long)p.nbz * p.nby));
        const int lz = threadIdx.x & (kBZ - 1);
        const int ly = (threadIdx.x >> 4) & (kBY - 1);
        const int lx = threadIdx.x >> 6;
        xl = bx * kBX + lx; y = by * kBY + ly; z = bz * kBZ + lz;
        inb = (xl < p.nx) && (y < p.Y) && (z < p.Z);
    }
    const double px = (double)(p.x0 + xl), py = (double)y, pz = (double)z;
    const size_t off = ((size_t)xl * p.Y + y) * p.Z + z;
    double bd[KS];
    int bi[KS];
    double wg[KS];
    double wi;
    if (MODE >= 2) {
        if (!inb) return;
        unsigned short id[KS];
        if (KS == 4 && p.k == 4) {
            const uint2 v = *reinterpret_cast<const uint2 *>(knn_cache + off * 4);
            id[0] = (unsigned short)(v.x & 0xffffu); id[1] = (unsigned short)(v.x >> 16);
            id[2] = (unsigned short)(v.y & 0xffffu); id[3] = (unsigned short)(v.y >> 16);
        } else {
#pragma unroll
            for (int j = 0; j < KS; ++j) id[j] = j < p.k ? knn_cache[off * p.k + j] : (unsigned short)0;
        }
#pragma unroll
        for (int j = 0; j < KS; ++j) bi[j] = min((int)id[j], p.N - 1);          // a stale or foreign workspace must not fault
#pragma unroll
        for (int j = 0; j < KS; ++j) {
            const int gi = bi[j];
            const double dx = px - node_pos[3 * gi], dy = py - node_pos[3 * gi + 1], dz = pz - node_pos[3 * gi + 2];
            bd[j] = (dx * dx + dy * dy) + dz * dz;
        }
    } else {
        block_knn<KS>(node_pos, cand + brick * (kCap + 1), p.N, px, py, pz, inb, bd, bi);
        if (!inb) return;
        if (MODE == 1) {
            if (KS == 4 && p.k == 4) {
                uint2 v;
                v.x = (unsigned)bi[0] | ((unsigned)bi[1] << 16);
                v.y = (unsigned)bi[2] | ((unsigned)bi[3] << 16);
                *reinterpret_cast<uint2 *>(knn_cache + off * 4) = v;
            } else {
#pragma unroll
                for (int j = 0; j < KS; ++j) if (j < p.k) knn_cache[off * p.k + j] = (unsigned short)bi[j];
            }
        }
    }
    dqb_weights<KS>(node_w, bd, bi, p.k, wg, wi);
    const D3 q = dqb_blend_warp<KS>(node_dq, wg, bi, p.k, p.lw.q, px, py, pz);          // fusion.py:178

    // ---- the views, in order: T and w stay in registers, rounded to the volume's dtype after every view
    VolT t = tsdf[off], w = tsdf_w[off];
    bool any = false;
    for (int view = 0; view < vw.n; ++view) {
        double sd;
        if (!warped_view_sd<DepthT, PINHOLE>(vw, vw.v[view], q, p.tdist, sd)) continue;
        const double m = sd < p.tdist ? sd : p.tdist;                                   // min(tdist, sd)
        const double tv = (double)t;
        double nw;
        if (vw.weight_mode == DFH_WARPED_W_UNIT) {
            const double wt = (double)w;
            t = (VolT)((vw.scale * tv * wt + m) / (vw.scale * (1.0 + wt)));             // fusion_dm.py:209
            nw = 1.0 + wt;                                                              // :210
        } else {
            double wt = (double)w;
            if (wt == 0.0) wt = wi;                                                     // fusion.py:186-187
            t = (VolT)((tv * wt + (m / vw.scale) * wi) / (wi + wt));                    // :189, sd in the volume's units
            nw = wi + wt;                                                               // :190
        }
        w = (VolT)(nw < p.wmax ? nw : p.wmax);
        any = true;
    }
    if (!any) return;
    tsdf[off] = t;
    tsdf_w[off] = w;
}

template <typename VolT, typename DepthT, bool PINHOLE>
static int launch_warped(const dfh_volume &vol, const dfh_nodes &nodes, int *cand, unsigned short *knn_cache, int mode,
                         const DqbParams &p, const WarpedViews &vw, hipStream_t s) {
    const long nbricks = (long)p.nbx * p.nby * p.nbz;
    const long nblocks = mode >= 2 ? ((long)p.nx * p.Y * p.Z + 255) / 256 : nbricks;
#define DFH_K1W(KS, MODE) hipLaunchKernelGGL((integrate_depth_dqb_kernel<VolT, DepthT, KS, MODE, PINHOLE>), dim3((unsigned)nblocks), dim3(256), \
                                             0, s, (VolT *)vol.tsdf, (VolT *)vol.tsdf_w, nodes.pos, nodes.dq, nodes.w, cand, knn_cache, p, vw)
    if (p.k <= 4) {                                   // 4 register slots suffice, as in K3
        if (mode == 0) DFH_K1W(4, 0); else if (mode == 1) DFH_K1W(4, 1); else DFH_K1W(4, 2);
    } else {
        if (mode == 0) DFH_K1W(kKMax, 0); else if (mode == 1) DFH_K1W(kKMax, 1); else DFH_K1W(kKMax, 2);
    }
#undef DFH_K1W
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

template <typename VolT, typename DepthT>
static int launch_warped_k(const dfh_volume &vol, const dfh_nodes &nodes, int *cand, unsigned short *knn_cache, int mode,
                           const DqbParams &p, const WarpedViews &vw, bool pinhole, hipStream_t s) {
    if (pinhole) return launch_warped<VolT, DepthT, true>(vol, nodes, cand, knn_cache, mode, p, vw, s);
    return launch_warped<VolT, DepthT, false>(vol, nodes, cand, knn_cache, mode, p, vw, s);
}

}  // namespace dfh

extern "C" int dfh_integrate_depth_dqb(const dfh_volume *vol, const dfh_depth_views *views, const dfh_nodes *nodes,
                                       const double lw_dq[8], double tdist, double wmax, int weight_mode, void *workspace,
                                       size_t workspace_bytes, int rebuild_candidates, void *stream) {
    using namespace dfh;
    static const char *const me = "dfh_integrate_depth_dqb";
    const int rc = check_volume(me, vol);
    if (rc != DFH_OK) return rc;
    DFH_REQUIRE(views && nodes && lw_dq, "%s: null pointer", me);
    DFH_REQUIRE(nodes->pos && nodes->dq && nodes->w, "%s: null node array", me);
    DFH_REQUIRE(views->n_views >= 0 && views->n_views <= kWarpedMaxViews, "%s: %d views (at most %d per call)", me, views->n_views,
                kWarpedMaxViews);
    if (views->n_views > 0) {
        DFH_REQUIRE(views->depth && views->lw, "%s: null pointer", me);
        for (int i = 0; i < views->n_views; ++i) DFH_REQUIRE(views->depth[i], "%s: depth map %d is null", me, i);
    }
    DFH_REQUIRE(views->H >= 2 && views->W >= 2 && (long)views->H * views->W < (1L << 31), "%s: bad depth map size %dx%d", me, views->H,
                views->W);
    DFH_REQUIRE(views->depth_dtype == DFH_F32 || views->depth_dtype == DFH_F64, "%s: bad depth_dtype %d", me, views->depth_dtype);
    DFH_REQUIRE(views->scale != 0.0, "%s: scale is 0", me);
    const int knn = nodes->knn, n_nodes = nodes->n_nodes;
    DFH_REQUIRE(knn >= 1 && knn <= kKMax, "%s: knn=%d outside [1,%d]", me, knn, kKMax);
    DFH_REQUIRE(n_nodes >= knn, "%s: %d nodes < knn=%d", me, n_nodes, knn);
    DFH_REQUIRE(weight_mode == DFH_WARPED_W_UNIT || weight_mode == DFH_WARPED_W_NODE_DISTANCE, "%s: bad weight_mode %d", me, weight_mode);
    const dfh_slab *sl = &vol->slab;
    if (sl->x1 == sl->x0 || views->n_views == 0) return DFH_OK;
    DFH_REQUIRE(workspace && workspace_bytes >= dfh_dqb_workspace_bytes(sl), "%s: workspace too small (need %zu bytes)", me,
                dfh_dqb_workspace_bytes(sl));
    DqbParams p = dqb_params(*sl, nullptr, n_nodes, knn);
    for (int i = 0; i < 8; ++i) p.lw.q[i] = lw_dq[i];
    p.tdist = tdist; p.wmax = wmax;
    DFH_REQUIRE((long)p.nbx * p.nby * p.nbz < (1L << 31), "%s: too many bricks", me);
    WarpedViews vw = {};
    for (int i = 0; i < 9; ++i) { vw.K.m[i] = views->K[i]; vw.Kinv.m[i] = views->Kinv[i]; }
    vw.scale = views->scale; vw.cx = views->center[0]; vw.cy = views->center[1]; vw.cz = views->center[2];
    vw.half = (double)views->tsdf_res / 2.0;             // np.zeros(3) + tsdf_res/2 (fusion_dm.py:183)
    vw.H = views->H; vw.W = views->W; vw.n = views->n_views; vw.weight_mode = weight_mode;
    for (int v = 0; v < views->n_views; ++v) {
        for (int i = 0; i < 12; ++i) vw.v[v].lw[i] = views->lw[12 * v + i];
        vw.v[v].depth = views->depth[v];
    }
    const double *K = views->K, *Kinv = views->Kinv;       // the pinhole test of dfh_integrate_depth (fill_params)
    const bool pinhole = K[1] == 0.0 && K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0 && Kinv[6] == 0.0 && Kinv[7] == 0.0 &&
                         Kinv[8] == 1.0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int *cand = static_cast<int *>(workspace);
    // the index region of a dfh_dqb_workspace_bytes_cached() buffer, where dfh_fuse_volume_dqb keeps it
    const size_t base = cand_bytes(*sl);
    const size_t cached1 = dfh_dqb_workspace_bytes_cached(sl, knn, n_nodes, 1);
    const bool has_idx = cached1 > base && workspace_bytes >= cached1 && !on(opt().k3_no_cache);
    unsigned short *knn_cache = has_idx ? reinterpret_cast<unsigned short *>(static_cast<char *>(workspace) + base) : nullptr;
    const int mode = !has_idx ? 0 : (rebuild_candidates ? 1 : 2);
    if (rebuild_candidates) {
        const int rb = dfh_dqb_build_candidates(sl, nodes->pos, n_nodes, knn, workspace, workspace_bytes, stream);
        if (rb != DFH_OK) return rb;
        if (has_idx) dqb_forget_weights(workspace);
    }
    const bool v32 = vol->dtype == DFH_F32, d32 = views->depth_dtype == DFH_F32;
    if (v32) {
        if (d32) return launch_warped_k<float, float>(*vol, *nodes, cand, knn_cache, mode, p, vw, pinhole, s);
        return launch_warped_k<float, double>(*vol, *nodes, cand, knn_cache, mode, p, vw, pinhole, s);
    }
    if (d32) return launch_warped_k<double, float>(*vol, *nodes, cand, knn_cache, mode, p, vw, pinhole, s);
    return launch_warped_k<double, double>(*vol, *nodes, cand, knn_cache, mode, p, vw, pinhole, s);
}
