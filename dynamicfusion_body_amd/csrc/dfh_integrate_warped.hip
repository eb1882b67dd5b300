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
// The search, the blend weights and the blended double warp are the functions K3's exact kernel calls (dfh_dqb_front.h).  The
// views table, the projection chain (exact_voxel of dfh_integrate.hip at a double position), the voxel decodes and the stored
// node indices are shared with the colour fusion: dfh_warped_views.h.  This file holds what is K1w's own: the T / w update per
// view with its two weight rules, the launch table and the entry point.
#include "dfh_warped_views.h"

namespace dfh {

void dqb_forget_weights(const void *workspace);        // dfh_fuse_volume.hip

struct WarpedViews {
    WarpViewsHead h;
    int weight_mode;
    WarpView v[kMaxWarpViews];
};

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
    // ---- which voxel, which nodes
    int xl, y, z;
    size_t off;
    bool inb;
    if (MODE >= 2) {
        if (!zrun_offset(p, off)) return;
        inb = true;
        zrun_voxel(p, off, xl, y, z);
    } else {
        inb = brick_voxel(p, blockIdx.x, xl, y, z);
        off = voxel_offset(p, xl, y, z);
    }
    const double px = (double)(p.x0 + xl), py = (double)y, pz = (double)z;
    double bd[KS];
    int bi[KS];
    double wg[KS];
    double wi;
    if (MODE >= 2) {
        load_stored_knn<KS>(knn_cache, off, p, node_pos, px, py, pz, bd, bi);
    } else {
        block_knn<KS>(node_pos, cand + (size_t)blockIdx.x * (kCap + 1), p.N, px, py, pz, inb, bd, bi);
        if (!inb) return;
        if (MODE == 1) store_knn<KS>(knn_cache, off, p, bi);
    }
    dqb_weights<KS>(node_w, bd, bi, p.k, wg, wi);
    const D3 q = dqb_blend_warp<KS>(node_dq, wg, bi, p.k, p.lw.q, px, py, pz);          // fusion.py:178

    // ---- the views, in order: T and w stay in registers, rounded to the volume's dtype after every view
    VolT t = tsdf[off], w = tsdf_w[off];
    bool any = false;
    for (int view = 0; view < vw.h.n; ++view) {
        double sd;
        size_t pix;
        if (!warped_view_sd<PINHOLE>(vw.h, vw.v[view], q, p.tdist, sizeof(DepthT) == 8, sd, pix)) continue;
        const double m = sd < p.tdist ? sd : p.tdist;                                   // min(tdist, sd)
        const double tv = (double)t;
        double nw;
        if (vw.weight_mode == DFH_WARPED_W_UNIT) {
            const double wt = (double)w;
            t = (VolT)((vw.h.scale * tv * wt + m) / (vw.h.scale * (1.0 + wt)));         // fusion_dm.py:209
            nw = 1.0 + wt;                                                              // :210
        } else {
            double wt = (double)w;
            if (wt == 0.0) wt = wi;                                                     // fusion.py:186-187
            t = (VolT)((tv * wt + (m / vw.h.scale) * wi) / (wi + wt));                  // :189, sd in the volume's units
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
    int rv = check_views_maps(me, views, true);
    if (rv == DFH_OK) rv = check_views_geometry(me, views);
    if (rv == DFH_OK) rv = check_knn(me, nodes);
    if (rv != DFH_OK) return rv;
    const int knn = nodes->knn, n_nodes = nodes->n_nodes;
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
    fill_views(vw.h, vw.v, views);
    vw.weight_mode = weight_mode;
    const bool pinhole = is_pinhole(views->K, views->Kinv);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int *cand = static_cast<int *>(workspace);
    unsigned short *knn_cache = dqb_index_region(sl, knn, n_nodes, workspace, workspace_bytes);
    const int mode = !knn_cache ? 0 : (rebuild_candidates ? 1 : 2);      // no index region: search every time
    if (rebuild_candidates) {
        const int rb = dfh_dqb_build_candidates(sl, nodes->pos, n_nodes, knn, workspace, workspace_bytes, stream);
        if (rb != DFH_OK) return rb;
        if (knn_cache) dqb_forget_weights(workspace);
    }
    const bool v32 = vol->dtype == DFH_F32, d32 = views->depth_dtype == DFH_F32;
    if (v32) {
        if (d32) return launch_warped_k<float, float>(*vol, *nodes, cand, knn_cache, mode, p, vw, pinhole, s);
        return launch_warped_k<float, double>(*vol, *nodes, cand, knn_cache, mode, p, vw, pinhole, s);
    }
    if (d32) return launch_warped_k<double, float>(*vol, *nodes, cand, knn_cache, mode, p, vw, pinhole, s);
    return launch_warped_k<double, double>(*vol, *nodes, cand, knn_cache, mode, p, vw, pinhole, s);
}
