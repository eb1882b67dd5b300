// K18: the photometric term of the warp-field solve -- one colour-consistency row per sample (include/dfusion_hip.h:
// dfh_gn_photometric; restated in tests/photometric_np.py).
//
// A photo sample is a canonical point with a reference intensity: it is warped, projected into the frame's views, depth-gated as
// the colour fusion gates a voxel (K17), and the row I(u, v) - ref of the view it lies closest to the observed surface in is
// differentiated through the bilinear cell it falls into.  The row is point_row with g = dI/dx', the image gradient pulled back
// through the projection, and the rows go the way of every sparse term (dfh_gn_term_rows.h).  There is one row per sample, so a
// tile is staged whole: one Jacobian row per thread at its compacted place, every run's Gram matrix in one pass.
#include "dfh_gn_term_rows.h"

#include <cmath>

namespace dfh {

struct PhotoParams {
    Mat3 K, Kinv;
    DQ lw;
    double scale, cx, cy, cz, half;
    double weight, huber, max_diff, band_sd;
    int H, W, n_views, depth_f64, n;
    const AssocView *views;
    const unsigned *color[DFH_GN_MAX_VIEWS];      // indexed by the (uniform) view loop only
};

// luma of one RGBX pixel: the integer numerator makes it exact
__device__ __forceinline__ double photo_luma(unsigned rgbx) {
    return (double)(77u * (rgbx & 0xffu) + 150u * ((rgbx >> 8) & 0xffu) + 29u * ((rgbx >> 16) & 0xffu)) / 256.0;
}

// Steps 2-4 and 6 of dfusion_hip.h for one warped sample: the view it lies closest to the observed surface in (-1: none passed),
// the interpolated intensity there and its gradient g with respect to x'.
__device__ __forceinline__ int photo_views(const PhotoParams &p, const D3 &xp, double &I_out, double (&g)[3]) {
    int best_view = -1;
    double best = __builtin_huge_val();
    I_out = 0.0; g[0] = 0.0; g[1] = 0.0; g[2] = 0.0;
    const double wx = p.scale * (xp.x - p.half) + p.cx, wy = p.scale * (xp.y - p.half) + p.cy, wz = p.scale * (xp.z - p.half) + p.cz;
    for (int view = 0; view < p.n_views; ++view) {                   // (uniform: the views' parameters come through scalar loads)
        const double *lw = p.views[view].lw_cam;
        const double l0 = ((lw[0] * wx + lw[1] * wy) + lw[2] * wz) + lw[3];
        const double l1 = ((lw[4] * wx + lw[5] * wy) + lw[6] * wz) + lw[7];
        const double l2 = ((lw[8] * wx + lw[9] * wy) + lw[10] * wz) + lw[11];
        const double a = (p.K.m[0] * l0 + p.K.m[1] * l1) + p.K.m[2] * l2;
        const double b = (p.K.m[3] * l0 + p.K.m[4] * l1) + p.K.m[5] * l2;
        const double c = (p.K.m[6] * l0 + p.K.m[7] * l1) + p.K.m[8] * l2;
        if (!(c != 0.0)) continue;
        const double u = a / c, v = b / c;
        // (a warped position that is not finite fails here: every comparison with a NaN is false)
        if (!((u >= 0.0) && (u < (double)(p.W - 1)) && (v >= 0.0) && (v < (double)(p.H - 1)))) continue;
        const size_t pix = (size_t)(int)rint(v) * p.W + (int)rint(u);      // 0 <= rint(u) <= W - 1, 0 <= rint(v) <= H - 1
        const void *dm = p.views[view].depth;
        const double z = -1.0 * (p.depth_f64 ? static_cast<const double *>(dm)[pix] : (double)static_cast<const float *>(dm)[pix]);
        if (!(z > 0.0)) continue;
        const double a0 = z * u, a1 = z * v;
        if (!((a0 < __builtin_huge_val()) & (a1 < __builtin_huge_val()))) continue;
        const double sd = ((p.Kinv.m[6] * a0 + p.Kinv.m[7] * a1) + p.Kinv.m[8] * (z * 1.0)) - l2;
        const double asd = fabs(sd);
        if (!(asd <= p.band_sd) || !(asd < best)) continue;            // (strict, in view order: ties go to the lower index)
        best = asd;
        best_view = view;
        // the bilinear cell: 0 <= i0 <= W - 2 and 0 <= j0 <= H - 2 by the visibility test, so all four taps lie in the image
        const int i0 = (int)floor(u), j0 = (int)floor(v);
        const double fu = u - (double)i0, fv = v - (double)j0;
        const unsigned *img = p.color[view] + (size_t)j0 * p.W + i0;
        const double Y00 = photo_luma(img[0]), Y10 = photo_luma(img[1]), Y01 = photo_luma(img[p.W]), Y11 = photo_luma(img[p.W + 1]);
        I_out = (1.0 - fv) * ((1.0 - fu) * Y00 + fu * Y10) + fv * ((1.0 - fu) * Y01 + fu * Y11);
        const double Iu = (1.0 - fv) * (Y10 - Y00) + fv * (Y11 - Y01);
        const double Iv = (1.0 - fu) * (Y01 - Y00) + fu * (Y11 - Y10);
        const double h0 = Iu * ((p.K.m[0] - u * p.K.m[6]) / c) + Iv * ((p.K.m[3] - v * p.K.m[6]) / c);
        const double h1 = Iu * ((p.K.m[1] - u * p.K.m[7]) / c) + Iv * ((p.K.m[4] - v * p.K.m[7]) / c);
        const double h2 = Iu * ((p.K.m[2] - u * p.K.m[8]) / c) + Iv * ((p.K.m[5] - v * p.K.m[8]) / c);
        g[0] = p.scale * ((h0 * lw[0] + h1 * lw[4]) + h2 * lw[8]);
        g[1] = p.scale * ((h0 * lw[1] + h1 * lw[5]) + h2 * lw[9]);
        g[2] = p.scale * ((h0 * lw[2] + h1 * lw[6]) + h2 * lw[10]);
    }
    return best_view;
}

// One kTile-sample tile per workgroup, one thread per sample; writes dfh_gn_problem.partial's layout: the tile's scratch rows, its
// {cost, 0} pair (tile_cost) and its rows' live flags (behind the n_tiles pairs).
template <int K>
__global__ __launch_bounds__(kTile) void gn_photo_rows_kernel(const double *__restrict__ spos, const int *__restrict__ nbr,
                                                              const double *__restrict__ wts, const double *__restrict__ ref,
                                                              const unsigned char *__restrict__ valid, const double *__restrict__ conf,
                                                              const double *__restrict__ node_dq, const PhotoParams p,
                                                              const int *__restrict__ run_id, double *__restrict__ partial,
                                                              double *__restrict__ tile_cost, int n_tiles,
                                                              unsigned char *__restrict__ active_out, int *__restrict__ view_out,
                                                              double *__restrict__ resid_out) {
    constexpr int NJ = 6 * K;                   // Jacobian entries per row
    constexpr int LD = NJ + 1;                  // + residual
    __shared__ double sJ[kTile * LD];           // the compacted samples' rows [J | r]
    __shared__ TermTile<kTileWaves> sT;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.x * kTile + tid;
    const int tile_n = min(kTile, p.n - blockIdx.x * kTile);
    // pass 1: warp, views, intensity, gate (steps 1-5)
    bool act = false;
    double obj = 0.0, r = 0.0, sc = 0.0, nb = 1.0;
    int idx[kKMaxS];
    double w[kKMaxS], bh[8], pf[3], g[3];
    if (tid < tile_n) {
#pragma unroll
        for (int j = 0; j < kKMaxS; ++j) {
            idx[j] = j < K ? nbr[(size_t)s * K + j] : 0;
            w[j] = j < K ? wts[(size_t)s * K + j] : 0.0;
        }
        nb = blend_static(node_dq, idx, w, K, bh);
        pf[0] = round_f32(spos[3 * (size_t)s]); pf[1] = round_f32(spos[3 * (size_t)s + 1]); pf[2] = round_f32(spos[3 * (size_t)s + 2]);
        const D3 x1 = dqb_warp_exact(bh, pf[0], pf[1], pf[2]);
        const D3 xp = dqb_warp_exact(p.lw.q, round_f32(x1.x), round_f32(x1.y), round_f32(x1.z));
        double I;
        const int view = photo_views(p, xp, I, g);
        r = I - ref[s];
        const double s2 = p.weight * (conf ? conf[s] : 1.0);
        act = (valid ? valid[s] != 0 : true) && s2 > 0.0 && view >= 0 && fabs(r) < __builtin_huge_val() &&      // (a NaN fails)
              (p.max_diff <= 0.0 || fabs(r) <= p.max_diff);
        if (act) robust_scale(r * r, s2, p.huber, obj, sc);          // scalar Huber on |r|
        if (active_out) active_out[s] = act ? 1 : 0;
        if (view_out) view_out[s] = act ? view : -1;
        if (resid_out) resid_out[s] = act ? r : 0.0;
    }
    int pos, n_valid, row_first, rows_tile;
    if (!term_tile_compact(sT, act, run_id, tile_n, tile_cost, n_tiles, pos, n_valid, row_first, rows_tile)) return;
    if (act) {                                                       // one Jacobian row per thread, at its compacted place
        sT.row[pos] = (unsigned short)(run_id[s] - row_first);
        double Jrow[NJ];
        point_row(node_dq, idx, w, K, p.lw.q, bh, nb, pf[0], pf[1], pf[2], g, sc, Jrow);
#pragma unroll
        for (int j = 0; j < NJ; ++j) sJ[pos * LD + j] = Jrow[j];
        sJ[pos * LD + NJ] = sc * r;
    }
    const int n_runs = term_tile_runs<K>(sT, obj, n_valid, row_first, rows_tile, partial, tile_cost, n_tiles);
    // Gram matrix of every run over X = the run's rows of [J | r] (n x (6K + 1)), whole and complete: one wave per run, runs dealt
    // round-robin.
    for (int rn = wv; rn < n_runs; rn += kTileWaves) {
        const int t0 = sT.run[rn], t1 = sT.run[rn + 1];
        gram_run<K, false>(sJ, t0, t1, false, true, partial + (size_t)(row_first + sT.row[t0]) * gn_row_stride(K), lane);
    }
}

int gn_add_photometric_impl(const dfh_gn_problem &q, const dfh_gn_frame &f, const dfh_gn_photometric &t, void *stream) {
    if (t.n == 0 || t.weight == 0.0) return DFH_OK;                  // nothing to add: no launch, the system stays as it is
    PhotoParams p;
    for (int i = 0; i < 9; ++i) { p.K.m[i] = f.K[i]; p.Kinv.m[i] = f.Kinv[i]; }
    for (int i = 0; i < 8; ++i) p.lw.q[i] = q.lw_dq[i];
    p.scale = f.scale; p.cx = f.center[0]; p.cy = f.center[1]; p.cz = f.center[2]; p.half = f.half;
    p.weight = t.weight; p.huber = t.huber_delta; p.max_diff = t.max_diff; p.band_sd = t.band_sd;
    p.H = f.H; p.W = f.W; p.n_views = f.n_views; p.depth_f64 = f.depth_dtype == DFH_F64 ? 1 : 0; p.n = t.n;
    p.views = static_cast<const AssocView *>(f.views);
    for (int v = 0; v < DFH_GN_MAX_VIEWS; ++v) p.color[v] = v < f.n_views ? static_cast<const unsigned *>(t.color[v]) : nullptr;
    return term_add(q, term_plan(t), t.n, stream, [&](auto kk, dim3 grid, double *tile_cost, int n_tiles) {
        hipLaunchKernelGGL(gn_photo_rows_kernel<decltype(kk)::value>, grid, dim3(kTile), 0, (hipStream_t)stream, t.pos, t.nbr, t.weights,
                           t.ref, t.valid, t.conf, q.node_dq, p, t.run_id, t.partial, tile_cost, n_tiles, t.active_out, t.view_out,
                           t.resid_out);
    });
}

}  // namespace dfh

extern "C" {

int dfh_gn_add_photometric(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_photometric *photo, void *stream) {
    using namespace dfh;
    int rc = check_problem("dfh_gn_add_photometric", problem, true);
    if (rc == DFH_OK) rc = check_photometric("dfh_gn_add_photometric", photo, frame, false);
    if (rc != DFH_OK) return rc;
    return gn_add_photometric_impl(*problem, *frame, *photo, stream);
}

}  // extern "C"
