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
// The search, the blend weights and the blended double warp are the functions K3 and K1w call (dfh_dqb_front.h).  The views
// table, the projection chain, the voxel decodes and the stored-index load are shared with K1w: dfh_warped_views.h.  This file
// holds what is K17's own: the canonical gate with its block-wide OR, the view gate, the colour mean, sample_colors, the launch
// table and the entry points.
#include "dfh_warped_views.h"

namespace dfh {

// K1w's table plus the gates and the colour images: 2.1 KB by value in the kernel-argument segment, read through scalar loads
struct ColorViews {
    WarpViewsHead h;
    double band_vox, band_sd;
    int vol_f64, depth_f64;
    WarpView v[kMaxWarpViews];
    const unsigned *color[kMaxWarpViews];       // H x W RGBX pixels, view by view
};

// MODE 0: no nodes, q = i; 1: search the brick's candidates; 2: load the stored indices.
template <int KS, int MODE, bool PINHOLE>
__global__ __launch_bounds__(256) void integrate_color_kernel(float4 *__restrict__ C, const void *__restrict__ tsdf,
                                                               const void *__restrict__ tsdf_w,
                                                               const double *__restrict__ node_pos,
                                                               const double *__restrict__ node_dq,
                                                               const double *__restrict__ node_w, const int *__restrict__ cand,
                                                               const unsigned short *__restrict__ knn_cache, const DqbParams p,
                                                               const ColorViews vw) {
    // ---- which voxel.  Along z the gate needs no decode: the 64-bit divisions wait until the lane is known to be live.
    int xl = 0, y = 0, z = 0;
    bool inb;
    size_t off;
    if (MODE != 1) {
        inb = zrun_offset(p, off);
    } else {
        inb = brick_voxel(p, blockIdx.x, xl, y, z);
        off = voxel_offset(p, xl, y, z);
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
        zrun_voxel(p, off, xl, y, z);
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
            load_stored_knn<KS>(knn_cache, off, p, node_pos, px, py, pz, bd, bi);
        } else {
            block_knn<KS>(node_pos, cand + (size_t)blockIdx.x * (kCap + 1), p.N, px, py, pz, live, bd, bi);
            if (!live) return;
        }
        dqb_weights<KS>(node_w, bd, bi, p.k, wg, wi);
        q = dqb_blend_warp<KS>(node_dq, wg, bi, p.k, p.lw.q, px, py, pz);
    }

    // ---- the views, in order: C stays in registers, rounded to float32 after every view
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    bool any = false;
    for (int view = 0; view < vw.h.n; ++view) {
        double sd;
        size_t pix;
        if (!warped_view_sd<PINHOLE>(vw.h, vw.v[view], q, p.tdist, vw.depth_f64 != 0, sd, pix)) continue;
        if (!(fabs(sd) <= vw.band_sd)) continue;                                       // the view gate
        if (!any) { c = C[off]; any = true; }
        const unsigned rgbx = vw.color[view][pix];
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
    int rv = check_views_maps(me, views, color != nullptr);
    if (rv != DFH_OK) return rv;
    for (int i = 0; i < views->n_views; ++i) DFH_REQUIRE(color[i], "%s: colour image %d is null", me, i);
    rv = check_views_geometry(me, views);
    if (rv == DFH_OK && nodes) rv = check_knn(me, nodes);
    if (rv != DFH_OK) return rv;
    const int knn = nodes ? nodes->knn : 0, n_nodes = nodes ? nodes->n_nodes : 0;
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
            size_t cached1;
            knn_cache = dqb_index_region(sl, knn, n_nodes, workspace, workspace_bytes, &cached1);
            DFH_REQUIRE(knn_cache, "%s: the workspace has no index region (need %zu bytes)", me, cached1);
            mode = 2;
        }
    }
    p.tdist = tdist; p.wmax = wmax;
    ColorViews vw = {};
    fill_views(vw.h, vw.v, views);
    vw.band_vox = band_vox; vw.band_sd = band_sd;
    vw.vol_f64 = vol->dtype == DFH_F64; vw.depth_f64 = views->depth_dtype == DFH_F64;
    for (int v = 0; v < views->n_views; ++v) vw.color[v] = static_cast<const unsigned *>(color[v]);
    const bool pinhole = is_pinhole(views->K, views->Kinv);
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
