// K17  colour: depth-registered colour images averaged into a per-voxel colour volume through the warp field
// (dfh_integrate_color), and the colour volume sampled at mesh vertices (dfh_sample_colors).  No reference counterpart: the
// reference reconstructs geometry only.  The semantics are written out operation by operation in include/dfusion_hip.h.
//
// dfh_integrate_color is K1w's chain (dfh_integrate_warped.hip) behind a canonical gate: only voxels inside a narrow band of
// the canonical surface (w > 0, |T| <= band_vox) are warped and projected at all, a few per cent of a volume.  One voxel per
// lane.  Without nodes and with stored node indices the threads run along z and a lane returns right after the gate; the
// searching mode runs K3's 4 x 4 x 16 bricks, the gate result is block_knn's `active` argument, and a workgroup without a live
// lane returns through one block-wide OR before it stages a candidate.  C is moved as one float4, a colour pixel is one dword at
// the index the depth gather computed.  The volume's and the depth maps' dtypes are wave-uniform branches at their single loads.
//
// The search, the blend weights and the blended double warp are the functions K3 and K1w call (dfh_dqb_front.h).  Restated here:
//   * the voxel decode and the stored-index load: integrate_depth_dqb_kernel's (dfh_integrate_warped.hip), modes 0 / 2 -- with
//     the decode of the z-running modes moved behind the gate (the offset is the thread's linear index; its three 64-bit
//     divisions in front of it cost the no-node sweep 12 of 57 us at 256^3) and the brick decode in 32 bits;
//   * the views' table and the projection chain: WarpedViews / warped_view_sd of dfh_integrate_warped.hip, statement for
//     statement, with the pixel index handed out and the depth dtype a run-time branch at the load.
#include "dfh_dqb_front.h"

namespace dfh {

constexpr int kColorMaxViews = 16;

struct ColorView {
    double lw[12];              // 3x4 row-major extrinsic
    const void *depth;          // H x W map of the call's depth dtype
    const unsigned *color;      // H x W RGBX pixels
};

// WarpedViews of dfh_integrate_warped.hip plus the colour pointers and the gates: 2.1 KB by value in the kernel-argument
// segment, read through scalar loads
struct ColorViews {
    Mat3 K, Kinv;
    double scale, cx, cy, cz, half;
    double band_vox, band_sd;
    int H, W, n;
    int vol_f64, depth_f64;
    ColorView v[kColorMaxViews];
};

// warped_view_sd of dfh_integrate_warped.hip (exact_voxel of dfh_integrate.hip at a double position): false = this view has no
// measurement for the voxel; sd_out = the signed distance and pix_out = vi * W + ui where it has.
template <bool PINHOLE>
__device__ __forceinline__ bool color_view_sd(const ColorViews &vw, const ColorView &view, const D3 &q, double tdist, double &sd_out,
                                              size_t &pix_out) {
    const double *lw = view.lw;
    const double px = vw.scale * (q.x - vw.half) + vw.cx;
    const double py = vw.scale * (q.y - vw.half) + vw.cy;
    const double pz = vw.scale * (q.z - vw.half) + vw.cz;
    const double l0 = ((lw[0] * px + lw[1] * py) + lw[2] * pz) + lw[3];
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
    if (!(p2 != 0.0)) return false;
    const double u = p0 / p2;
    const double v = p1 / p2;
    // (a warped position that is not finite fails here: every comparison with a NaN is false)
    if (!((u >= 0.0) && (u < (double)(vw.W - 1)) && (v >= 0.0) && (v < (double)(vw.H - 1)))) return false;
    const int ui = (int)rint(u);                                    // half to even; 0 <= ui <= W - 1, 0 <= vi <= H - 1
    const int vi = (int)rint(v);
    const size_t pix = (size_t)vi * vw.W + ui;
    const double dv = vw.depth_f64 ? static_cast<const double *>(view.depth)[pix] : (double)static_cast<const float *>(view.depth)[pix];
    const double zd = -1.0 * dv;
    if (!(zd > 0.0)) return false;
    double cz;
    if (PINHOLE) {
        cz = zd;                                                    // Kinv row 2 == [0,0,1]
        // ... unless z u or z v overflows: 0 * inf = NaN in the general chain, and a NaN sd passes nothing
        if (!((zd * u < __builtin_huge_val()) & (zd * v < __builtin_huge_val()))) return false;
    } else {
        cz = (vw.Kinv.m[6] * (zd * u) + vw.Kinv.m[7] * (zd * v)) + vw.Kinv.m[8] * (zd * 1.0);
    }
    const double sd = cz - l2;
    sd_out = sd;
    pix_out = pix;
    return sd > -1.0 * tdist;
}

// MODE 0: no nodes, q = i; 1: search the brick's candidates; 2: load the stored indices.
template <int KS, int MODE, bool PINHOLE>
__global__ __launch_bounds__(256) void integrate_color_kernel(float4 *__restrict__ C, const void *__restrict__ tsdf,
                                                               const void *__restrict__ tsdf_w,
                                                               const double *__restrict__ node_pos,
                                                               const double *__restrict__ node_dq,
                                                               const double *__restrict__ node_w, const int *__restrict__ cand,
                                                               const unsigned short *__restrict__ knn_cache, const DqbParams p,
                                                               const ColorViews vw) {
    // ---- which voxel: integrate_depth_dqb_kernel's decode (dfh_integrate_warped.hip).  Along z the voxel's offset IS the thread's
    // linear index, so the gate needs no decode: the 64-bit divisions wait until the lane is known to be live.
    const size_t nvox = (size_t)p.nx * p.Y * p.Z;
    const unsigned brick = blockIdx.x;          // (fewer than 2^31 bricks: checked by the host)
    int xl = 0, y = 0, z = 0;
    bool inb;
    size_t off;
    if (MODE != 1) {            // no search, no bricks: threads run along z
        off = (size_t)blockIdx.x * 256 + threadIdx.x;
        inb = off < nvox;
    } else {
        const unsigned bz = brick % (unsigned)p.nbz;
        const unsigned by = (brick / (unsigned)p.nbz) % (unsigned)p.nby;
        const unsigned bx = brick / ((unsigned)p.nbz * (unsigned)p.nby);
        const int lz = threadIdx.x & (kBZ - 1);
        const int ly = (threadIdx.x >> 4) & (kBY - 1);
        const int lx = threadIdx.x >> 6;
        xl = (int)bx * kBX + lx; y = (int)by * kBY + ly; z = (int)bz * kBZ + lz;
        inb = (xl < p.nx) && (y < p.Y) && (z < p.Z);
        off = ((size_t)xl * p.Y + y) * p.Z + z;
    }

    // ---- the canonical gate, before anything else
    bool live = false;
    if (inb) {
        double t, w;
        if (vw.vol_f64) {
            t = static_cast<const double *>(tsdf)[off];
            w = static_cast<const double *>(tsdf_w)[off];
        } else {
            t = (double)static_cast<const float *>(tsdf)[off];
            w = (double)static_cast<const float *>(tsdf_w)[off];
        }
        live = (w > 0.0) && (fabs(t) <= vw.band_vox);
    }
    if (MODE != 1) {
        if (!live) return;
        z = (int)(off % (size_t)p.Z);
        y = (int)((off / (size_t)p.Z) % (size_t)p.Y);
        xl = (int)(off / ((size_t)p.Z * p.Y));
    } else {
        if (!__syncthreads_or(live ? 1 : 0)) return;        // uniform: block_knn's barriers are reached by all or by none
    }

    // ---- the warped position: K1w's q
    const double px = (double)(p.x0 + xl), py = (double)y, pz = (double)z;
    D3 q;
    if (MODE == 0) {
        q.x = px; q.y = py; q.z = pz;
    } else {
        double bd[KS];
        int bi[KS];
        double wg[KS];
        double wi;
        if (MODE == 2) {
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
            block_knn<KS>(node_pos, cand + (size_t)brick * (kCap + 1), p.N, px, py, pz, live, bd, bi);
            if (!live) return;
        }
        dqb_weights<KS>(node_w, bd, bi, p.k, wg, wi);
        q = dqb_blend_warp<KS>(node_dq, wg, bi, p.k, p.lw.q, px, py, pz);
    }

    // ---- the views, in order: C stays in registers, rounded to float32 after every view
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    bool any = false;
    for (int view = 0; view < vw.n; ++view) {
        double sd;
        size_t pix;
        if (!color_view_sd<PINHOLE>(vw, vw.v[view], q, p.tdist, sd, pix)) continue;
        if (!(fabs(sd) <= vw.band_sd)) continue;                                       // the view gate
        if (!any) { c = C[off]; any = true; }
        const unsigned rgbx = vw.v[view].color[pix];
        const double wc = (double)c.w;
        const double den = wc + 1.0;
        c.x = (float)(((double)c.x * wc + (double)(rgbx & 0xffu)) / den);
        c.y = (float)(((double)c.y * wc + (double)((rgbx >> 8) & 0xffu)) / den);
        c.z = (float)(((double)c.z * wc + (double)((rgbx >> 16) & 0xffu)) / den);
        c.w = (float)(den < p.wmax ? den : p.wmax);
    }
    if (!any) return;
    C[off] = c;
}

template <bool PINHOLE>
static int launch_color(float4 *C, const dfh_volume &vol, const dfh_nodes *nodes, const int *cand, const unsigned short *knn_cache,
                        int mode, const DqbParams &p, const ColorViews &vw, hipStream_t s) {
    const long nbricks = (long)p.nbx * p.nby * p.nbz;
    const long nblocks = mode != 1 ? ((long)p.nx * p.Y * p.Z + 255) / 256 : nbricks;
    const double *npos = nodes ? nodes->pos : nullptr, *ndq = nodes ? nodes->dq : nullptr, *nw = nodes ? nodes->w : nullptr;
#define DFH_K17(KS, MODE) hipLaunchKernelGGL((integrate_color_kernel<KS, MODE, PINHOLE>), dim3((unsigned)nblocks), dim3(256), 0, s, C, \
                                             vol.tsdf, vol.tsdf_w, npos, ndq, nw, cand, knn_cache, p, vw)
    if (mode == 0) DFH_K17(4, 0);
    else if (p.k <= 4) { if (mode == 1) DFH_K17(4, 1); else DFH_K17(4, 2); }        // 4 register slots suffice, as in K3
    else { if (mode == 1) DFH_K17(kKMax, 1); else DFH_K17(kKMax, 2); }
#undef DFH_K17
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

// one point per lane; the semantics are those of include/dfusion_hip.h, statement for statement
__global__ __launch_bounds__(256) void sample_colors_kernel(const float4 *__restrict__ C, const double *__restrict__ points, long n,
                                                             int X, int Y, int Z, int x0, int x1, float *__restrict__ rgb_out,
                                                             unsigned char *__restrict__ valid_out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double p0 = points[3 * i], p1 = points[3 * i + 1], p2 = points[3 * i + 2];
    float r = 0.f, g = 0.f, b = 0.f;
    unsigned char valid = 0;
    // (a NaN fails every comparison; an infinity lies outside)
    const bool in = (p0 >= 0.0) && (p0 <= (double)(X - 1)) && (p1 >= 0.0) && (p1 <= (double)(Y - 1)) && (p2 >= 0.0) && (p2 <= (double)(Z - 1));
    if (in) {
        const int ix = max(min((int)floor(p0), X - 2), 0), iy = max(min((int)floor(p1), Y - 2), 0), iz = max(min((int)floor(p2), Z - 2), 0);
        const double fx = p0 - (double)ix, fy = p1 - (double)iy, fz = p2 - (double)iz;
        double S = 0.0, sr = 0.0, sg = 0.0, sb = 0.0;
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
            const int dx = corner >> 2, dy = (corner >> 1) & 1, dz = corner & 1;
            const int cx = ix + dx, cy = iy + dy, cz = iz + dz;
            if (cx < x0 || cx >= x1 || cy >= Y || cz >= Z) continue;
            const float4 c = C[((size_t)(cx - x0) * Y + cy) * Z + cz];
            if (!(c.w > 0.f)) continue;
            const double wx = dx ? fx : 1.0 - fx, wy = dy ? fy : 1.0 - fy, wz = dz ? fz : 1.0 - fz;
            const double tw = (wx * wy) * wz;
            S = S + tw;
            sr = sr + tw * (double)c.x;
            sg = sg + tw * (double)c.y;
            sb = sb + tw * (double)c.z;
        }
        if (S != 0.0) {
            r = (float)(sr / S); g = (float)(sg / S); b = (float)(sb / S);
            valid = 1;
        }
    }
    rgb_out[3 * i] = r; rgb_out[3 * i + 1] = g; rgb_out[3 * i + 2] = b;
    valid_out[i] = valid;
}

}  // namespace dfh

extern "C" int dfh_integrate_color(const dfh_color_volume *cvol, const dfh_volume *vol, const dfh_depth_views *views,
                                   const void *const *color, const dfh_nodes *nodes, const double lw_dq[8], double tdist,
                                   double band_vox, double band_sd, double wmax, void *workspace, size_t workspace_bytes,
                                   int use_stored_indices, void *stream) {
    using namespace dfh;
    static const char *const me = "dfh_integrate_color";
    DFH_REQUIRE(cvol && cvol->rgbw, "%s: null colour volume", me);
    const int rc = check_volume(me, vol);
    if (rc != DFH_OK) return rc;
    const dfh_slab *sl = &vol->slab;
    const dfh_slab *cs = &cvol->slab;
    DFH_REQUIRE(cs->res[0] == sl->res[0] && cs->res[1] == sl->res[1] && cs->res[2] == sl->res[2] && cs->x0 == sl->x0 && cs->x1 == sl->x1,
                "%s: the colour volume's slab is not the volume's", me);
    DFH_REQUIRE(views, "%s: null pointer", me);
    DFH_REQUIRE((nodes != nullptr) == (lw_dq != nullptr), "%s: nodes and lw_dq must both be given or both be null", me);
    if (nodes) DFH_REQUIRE(nodes->pos && nodes->dq && nodes->w, "%s: null node array", me);
    DFH_REQUIRE(views->n_views >= 0 && views->n_views <= kColorMaxViews, "%s: %d views (at most %d per call)", me, views->n_views,
                kColorMaxViews);
    if (views->n_views > 0) {
        DFH_REQUIRE(views->depth && views->lw && color, "%s: null pointer", me);
        for (int i = 0; i < views->n_views; ++i) DFH_REQUIRE(views->depth[i], "%s: depth map %d is null", me, i);
        for (int i = 0; i < views->n_views; ++i) DFH_REQUIRE(color[i], "%s: colour image %d is null", me, i);
    }
    DFH_REQUIRE(views->H >= 2 && views->W >= 2 && (long)views->H * views->W < (1L << 31), "%s: bad depth map size %dx%d", me, views->H,
                views->W);
    DFH_REQUIRE(views->depth_dtype == DFH_F32 || views->depth_dtype == DFH_F64, "%s: bad depth_dtype %d", me, views->depth_dtype);
    DFH_REQUIRE(views->scale != 0.0, "%s: scale is 0", me);
    int knn = 0, n_nodes = 0;
    if (nodes) {
        knn = nodes->knn; n_nodes = nodes->n_nodes;
        DFH_REQUIRE(knn >= 1 && knn <= kKMax, "%s: knn=%d outside [1,%d]", me, knn, kKMax);
        DFH_REQUIRE(n_nodes >= knn, "%s: %d nodes < knn=%d", me, n_nodes, knn);
    }
    DFH_REQUIRE(band_vox > 0.0 && band_sd > 0.0, "%s: band_vox and band_sd must be > 0", me);
    DFH_REQUIRE(wmax >= 1.0, "%s: wmax must be >= 1", me);
    DFH_REQUIRE(!use_stored_indices || nodes, "%s: stored indices need nodes", me);
    if (sl->x1 == sl->x0 || views->n_views == 0) return DFH_OK;
    DqbParams p = dqb_params(*sl, nullptr, n_nodes, knn);
    DFH_REQUIRE((long)p.nbx * p.nby * p.nbz < (1L << 31), "%s: too many bricks", me);
    DFH_REQUIRE(((long)p.nx * p.Y * p.Z + 255) / 256 < (1L << 31), "%s: too many voxels", me);
    const int *cand = nullptr;
    const unsigned short *knn_cache = nullptr;
    int mode = 0;
    if (nodes) {
        DFH_REQUIRE(workspace && workspace_bytes >= dfh_dqb_workspace_bytes(sl), "%s: workspace too small (need %zu bytes)", me,
                    dfh_dqb_workspace_bytes(sl));
        for (int i = 0; i < 8; ++i) p.lw.q[i] = lw_dq[i];
        cand = static_cast<const int *>(workspace);
        mode = 1;
        if (use_stored_indices) {
            // the index region of a dfh_dqb_workspace_bytes_cached() buffer, where dfh_fuse_volume_dqb and K1w keep it
            const size_t base = cand_bytes(*sl);
            const size_t cached1 = dfh_dqb_workspace_bytes_cached(sl, knn, n_nodes, 1);
            const bool has_idx = cached1 > base && workspace_bytes >= cached1 && !on(opt().k3_no_cache);
            DFH_REQUIRE(has_idx, "%s: the workspace has no index region (need %zu bytes)", me, cached1);
            knn_cache = reinterpret_cast<const unsigned short *>(static_cast<const char *>(workspace) + base);
            mode = 2;
        }
    }
    p.tdist = tdist; p.wmax = wmax;
    ColorViews vw = {};
    for (int i = 0; i < 9; ++i) { vw.K.m[i] = views->K[i]; vw.Kinv.m[i] = views->Kinv[i]; }
    vw.scale = views->scale; vw.cx = views->center[0]; vw.cy = views->center[1]; vw.cz = views->center[2];
    vw.half = (double)views->tsdf_res / 2.0;
    vw.band_vox = band_vox; vw.band_sd = band_sd;
    vw.H = views->H; vw.W = views->W; vw.n = views->n_views;
    vw.vol_f64 = vol->dtype == DFH_F64; vw.depth_f64 = views->depth_dtype == DFH_F64;
    for (int v = 0; v < views->n_views; ++v) {
        for (int i = 0; i < 12; ++i) vw.v[v].lw[i] = views->lw[12 * v + i];
        vw.v[v].depth = views->depth[v];
        vw.v[v].color = static_cast<const unsigned *>(color[v]);
    }
    const double *K = views->K, *Kinv = views->Kinv;       // the pinhole test of dfh_integrate_depth_dqb
    const bool pinhole = K[1] == 0.0 && K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0 && Kinv[6] == 0.0 && Kinv[7] == 0.0 &&
                         Kinv[8] == 1.0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float4 *C = reinterpret_cast<float4 *>(cvol->rgbw);
    if (pinhole) return launch_color<true>(C, *vol, nodes, cand, knn_cache, mode, p, vw, s);
    return launch_color<false>(C, *vol, nodes, cand, knn_cache, mode, p, vw, s);
}

extern "C" int dfh_sample_colors(const dfh_color_volume *cvol, const double *points, long n, float *rgb_out, unsigned char *valid_out,
                                 void *stream) {
    using namespace dfh;
    static const char *const me = "dfh_sample_colors";
    DFH_REQUIRE(cvol, "%s: null colour volume", me);
    const int rc = check_slab(me, &cvol->slab);
    if (rc != DFH_OK) return rc;
    DFH_REQUIRE(n >= 0 && n < (1L << 31), "%s: bad point count %ld", me, n);
    if (n == 0) return DFH_OK;
    DFH_REQUIRE(points && rgb_out && valid_out, "%s: null pointer", me);
    const dfh_slab &sl = cvol->slab;
    DFH_REQUIRE(cvol->rgbw || sl.x0 == sl.x1, "%s: null colour volume", me);
    hipLaunchKernelGGL(sample_colors_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4 *>(cvol->rgbw), points, n, sl.res[0], sl.res[1], sl.res[2], sl.x0, sl.x1, rgb_out,
                       valid_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}
