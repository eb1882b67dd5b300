// "Warp a canonical voxel and project it into the call's depth maps": what the depth fusion through the warp field (K1w,
// dfh_integrate_warped.hip) and the colour fusion (K17, dfh_color.hip) both run on top of K3's front end (dfh_dqb_front.h) -- the
// per-call views table, the projection chain at a double position, the voxel decodes, the stored node indices, and the host code
// that checks a dfh_depth_views, fills the table and finds a workspace's index region.  One statement of each: a fix to the pixel
// rule or to the pinhole chain's overflow guard is made here, for both.
// Relatives that stay where they are: exact_voxel (dfh_integrate.hip), the same chain at an integer voxel index on a 500-byte
// per-view block; the body of fuse_volume_dqb_kernel (dfh_fuse_volume.hip), whose register allocation moved when its decode was
// lifted; photo_views (dfh_photometric.hip), which always runs the general chain, guards unconditionally and picks a best view.
#pragma once
#include "dfh_dqb_front.h"

namespace dfh {

// ------------------------------------------------------------------------------- the views table
constexpr int kMaxWarpViews = 16;

struct WarpView {
    double lw[12];              // 3x4 row-major extrinsic
    const void *depth;          // H x W map of the call's depth dtype
};

// K, Kinv and the index -> world map.  With 16 x 104 B of views behind it a table is ~1.9 KB by value in the kernel-argument
// segment, read through scalar loads.
struct WarpViewsHead {
    Mat3 K, Kinv;
    double scale, cx, cy, cz, half;
    int H, W, n;
};

// exact_voxel of dfh_integrate.hip (fusion_dm.py:191-203, its operation order) at a double position q instead of an integer
// voxel index: false = this view has no measurement that updates the voxel; sd_out = the signed distance and pix_out = vi * W + ui
// where it has.  depth_f64: the maps' dtype, a compile-time constant (it folds) or a wave-uniform flag (a branch at the load).
template <bool PINHOLE>
__device__ __forceinline__ bool warped_view_sd(const WarpViewsHead &vw, const WarpView &view, const D3 &q, double tdist, bool depth_f64,
                                               double &sd_out, size_t &pix_out) {
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
    const int ui = (int)rint(u);                                    // Python round(): half to even (:196); 0 <= ui <= W - 1,
    const int vi = (int)rint(v);                                    // 0 <= vi <= H - 1
    const size_t pix = (size_t)vi * vw.W + ui;
    const double dv = depth_f64 ? static_cast<const double *>(view.depth)[pix] : (double)static_cast<const float *>(view.depth)[pix];
    const double zd = -1.0 * dv;
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
    pix_out = pix;
    return sd > -1.0 * tdist;                                       // :203
}

// ------------------------------------------------------------------------------- which voxel
// A workgroup = one of K3's 4 x 4 x 16 bricks (the searching modes; fewer than 2^31 bricks: checked by the host): false = the
// lane's voxel lies outside the slab.
__device__ __forceinline__ bool brick_voxel(const DqbParams &p, unsigned brick, int &xl, int &y, int &z) {
    const unsigned bz = brick % (unsigned)p.nbz;
    const unsigned by = (brick / (unsigned)p.nbz) % (unsigned)p.nby;
    const unsigned bx = brick / ((unsigned)p.nbz * (unsigned)p.nby);
    const int lz = threadIdx.x & (kBZ - 1);
    const int ly = (threadIdx.x >> 4) & (kBY - 1);
    const int lx = threadIdx.x >> 6;
    xl = (int)bx * kBX + lx; y = (int)by * kBY + ly; z = (int)bz * kBZ + lz;
    return (xl < p.nx) && (y < p.Y) && (z < p.Z);
}

__device__ __forceinline__ size_t voxel_offset(const DqbParams &p, int xl, int y, int z) { return ((size_t)xl * p.Y + y) * p.Z + z; }

// No search, no bricks: threads run along z (whole 128-B lines of every per-voxel array).  In two halves: a voxel's offset IS the
// thread's linear index, so a caller with a gate on the voxel's own values tests it first ...
__device__ __forceinline__ bool zrun_offset(const DqbParams &p, size_t &off) {
    off = (size_t)blockIdx.x * 256 + threadIdx.x;
    return off < (size_t)p.nx * p.Y * p.Z;
}

// ... and only its live lanes pay the three 64-bit divisions of the decode.
__device__ __forceinline__ void zrun_voxel(const DqbParams &p, size_t off, int &xl, int &y, int &z) {
    z = (int)(off % (size_t)p.Z);
    y = (int)((off / (size_t)p.Z) % (size_t)p.Y);
    xl = (int)(off / ((size_t)p.Z * p.Y));
}

// ------------------------------------------------------------------------------- the stored node indices
// The k node indices of the voxel at `off` from a workspace's index region (16-bit, k per voxel; k == 4: one packed 8-byte
// load) and their squared distances from (px, py, pz), recomputed.
template <int KS>
__device__ __forceinline__ void load_stored_knn(const unsigned short *__restrict__ knn_cache, size_t off, const DqbParams &p,
                                                const double *__restrict__ node_pos, double px, double py, double pz, double (&bd)[KS],
                                                int (&bi)[KS]) {
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
}

// ... and a search's result stored there
template <int KS>
__device__ __forceinline__ void store_knn(unsigned short *__restrict__ knn_cache, size_t off, const DqbParams &p, const int (&bi)[KS]) {
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

// ------------------------------------------------------------------------------- host side
// What both entry points check of their dfh_depth_views, in the order they have always reported it, in two functions: a call's
// own per-view pointers (K17's colour images) are checked between them.  First the count and the maps (`others`: the call's
// further per-view arrays are all there) ...
inline int check_views_maps(const char *me, const dfh_depth_views *views, bool others) {
    DFH_REQUIRE(views->n_views >= 0 && views->n_views <= kMaxWarpViews, "%s: %d views (at most %d per call)", me, views->n_views,
                kMaxWarpViews);
    if (views->n_views > 0) {
        DFH_REQUIRE(views->depth && views->lw && others, "%s: null pointer", me);
        for (int i = 0; i < views->n_views; ++i) DFH_REQUIRE(views->depth[i], "%s: depth map %d is null", me, i);
    }
    return DFH_OK;
}

// ... then the maps' size and dtype and the scale
inline int check_views_geometry(const char *me, const dfh_depth_views *views) {
    DFH_REQUIRE(views->H >= 2 && views->W >= 2 && (long)views->H * views->W < (1L << 31), "%s: bad depth map size %dx%d", me, views->H,
                views->W);
    DFH_REQUIRE(views->depth_dtype == DFH_F32 || views->depth_dtype == DFH_F64, "%s: bad depth_dtype %d", me, views->depth_dtype);
    DFH_REQUIRE(views->scale != 0.0, "%s: scale is 0", me);
    return DFH_OK;
}

inline int check_knn(const char *me, const dfh_nodes *nodes) {
    DFH_REQUIRE(nodes->knn >= 1 && nodes->knn <= kKMax, "%s: knn=%d outside [1,%d]", me, nodes->knn, kKMax);
    DFH_REQUIRE(nodes->n_nodes >= nodes->knn, "%s: %d nodes < knn=%d", me, nodes->n_nodes, nodes->knn);
    return DFH_OK;
}

inline void fill_views(WarpViewsHead &h, WarpView *v, const dfh_depth_views *views) {
    for (int i = 0; i < 9; ++i) { h.K.m[i] = views->K[i]; h.Kinv.m[i] = views->Kinv[i]; }
    h.scale = views->scale; h.cx = views->center[0]; h.cy = views->center[1]; h.cz = views->center[2];
    h.half = (double)views->tsdf_res / 2.0;             // np.zeros(3) + tsdf_res/2 (fusion_dm.py:183)
    h.H = views->H; h.W = views->W; h.n = views->n_views;
    for (int j = 0; j < views->n_views; ++j) {
        for (int i = 0; i < 12; ++i) v[j].lw[i] = views->lw[12 * j + i];
        v[j].depth = views->depth[j];
    }
}

// K = [[fx,0,cx],[0,fy,cy],[0,0,1]] and Kinv's last row (0,0,1): the terms the PINHOLE chains drop are exact zeros
inline bool is_pinhole(const double *K, const double *Kinv) {
    return K[1] == 0.0 && K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0 && Kinv[6] == 0.0 && Kinv[7] == 0.0 &&
           Kinv[8] == 1.0;
}

// The index region of a dfh_dqb_workspace_bytes_cached() buffer -- every voxel's k node indices, where dfh_fuse_volume_dqb and
// K1w keep them and K17 reads them -- or null when the workspace has none; *cached1_out = the bytes a workspace with one has.
inline unsigned short *dqb_index_region(const dfh_slab *sl, int knn, int n_nodes, void *workspace, size_t workspace_bytes,
                                        size_t *cached1_out = nullptr) {
    const size_t base = cand_bytes(*sl);
    const size_t cached1 = dfh_dqb_workspace_bytes_cached(sl, knn, n_nodes, 1);
    if (cached1_out) *cached1_out = cached1;
    const bool has_idx = cached1 > base && workspace_bytes >= cached1 && !on(opt().k3_no_cache);
    return has_idx ? reinterpret_cast<unsigned short *>(static_cast<char *>(workspace) + base) : nullptr;
}

}  // namespace dfh
