// K18: the photometric term of the warp-field solve -- one colour-consistency row per sample (include/dfusion_hip.h:
// dfh_gn_photometric; restated in tests/photometric_np.py).
//
// A photo sample is a canonical point with a reference intensity: it is warped, projected into the frame's views, depth-gated as
// the colour fusion gates a voxel (K17), and the row I(u, v) - ref of the view it lies closest to the observed surface in is
// differentiated through the bilinear cell it falls into.  The row has the form of one landmark row (dfh_landmarks.hip) with the
// axis e_a replaced by g = dI/dx', the image gradient pulled back through the projection; there is one row per sample, so a tile is
// one pass of gn_build_data_kernel's LDS layout: the tile's active samples compacted in order, one Jacobian row per thread, the Gram
// matrix of every run of equal node tuples on the fp64 matrix cores, STORED to the run's scratch row; gn_gather_kernel then adds the
// rows into the blocks with accumulate = true.  No floating-point atomics, the same bits every run.
#include "dfh_gn_rows.h"

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

// Jacobian row of I(x') with the gradient g = dI/dx' held constant: landmark_axis_row with the axis e_a replaced by g.
__device__ __forceinline__ void photo_row(const double *__restrict__ node_dq, const int *idx, const double *w, int k, const double *lwq,
                                          const double *bh, double nb, double pfx, double pfy, double pfz, const double *g, double sc,
                                          double *Jrow) {
    const Q4 rl{lwq[0], lwq[1], lwq[2], lwq[3]};
    const Q4 rlc = qconj(rl);
    const Q4 U = qmul(qmul(rlc, qpure(g[0], g[1], g[2])), rl);
    const Q4 Up = qpure(U.x, U.y, U.z);
    const Q4 rr{bh[0], bh[1], bh[2], bh[3]}, dd{bh[4], bh[5], bh[6], bh[7]};
    const Q4 Ur = qmul(Up, rr);
    Q4 g_r = qscale(qadd(qmul(Ur, qpure(pfx, pfy, pfz)), qmul(Up, dd)), -2.0);
    Q4 g_d = qscale(Ur, 2.0);
    const double gb = (g_r.w * bh[0] + g_r.x * bh[1] + g_r.y * bh[2] + g_r.z * bh[3]) +
                      (g_d.w * bh[4] + g_d.x * bh[5] + g_d.y * bh[6] + g_d.z * bh[7]);
    const double inv = 1.0 / nb;
    g_r = Q4{(g_r.w - gb * bh[0]) * inv, (g_r.x - gb * bh[1]) * inv, (g_r.y - gb * bh[2]) * inv, (g_r.z - gb * bh[3]) * inv};
    g_d = Q4{(g_d.w - gb * bh[4]) * inv, (g_d.x - gb * bh[5]) * inv, (g_d.y - gb * bh[6]) * inv, (g_d.z - gb * bh[7]) * inv};
#pragma unroll
    for (int j = 0; j < kKMaxS; ++j) {
        if (j < k) {
            const double *q = node_dq + 8 * idx[j];
            const Q4 rac{q[0], -q[1], -q[2], -q[3]}, dac{q[4], -q[5], -q[6], -q[7]};
            const Q4 ga = qadd(qmul(g_r, rac), qmul(g_d, dac));
            const Q4 t = qmul(g_d, rac);
            const double hw = 0.5 * w[j];
            Jrow[6 * j + 0] = sc * (hw * ga.x); Jrow[6 * j + 1] = sc * (hw * ga.y); Jrow[6 * j + 2] = sc * (hw * ga.z);
            Jrow[6 * j + 3] = sc * (hw * t.x); Jrow[6 * j + 4] = sc * (hw * t.y); Jrow[6 * j + 5] = sc * (hw * t.z);
        }
    }
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
    constexpr int ST_ = gn_row_stride(K);
    constexpr int NUP = gn_row_gram(K);
    __shared__ double sJ[kTile * LD];           // the compacted samples' rows [J | r]
    __shared__ int sWaveCnt[kTileWaves];
    __shared__ unsigned short sRow[kTile];      // scratch row of every compacted sample, relative to the tile's first
    __shared__ double sObj[kTileWaves];
    __shared__ int sRun[kTile + 1];
    __shared__ int sNRuns;
    __shared__ int sTouched[kTile];
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
        if (act) {
            const double q = r * r;
            if (p.huber > 0.0 && q > p.huber * p.huber) {              // scalar Huber on |r|
                const double n = sqrt(q);
                obj = s2 * p.huber * (n - 0.5 * p.huber);
                sc = sqrt(s2) * sqrt(p.huber / n);
            } else {
                obj = 0.5 * s2 * q;
                sc = sqrt(s2);
            }
        }
        if (active_out) active_out[s] = act ? 1 : 0;
        if (view_out) view_out[s] = act ? view : -1;
        if (resid_out) resid_out[s] = act ? r : 0.0;
    }
    // the active samples, compacted in order (gn_build_data_kernel's scheme)
    const unsigned long long bal = __ballot(act);
    if (lane == 0) sWaveCnt[wv] = __popcll(bal);
    __syncthreads();
    int pos = __popcll(bal & ((1ull << lane) - 1ull));
    for (int w_ = 0; w_ < wv; ++w_) pos += sWaveCnt[w_];
    int n_valid = 0;
#pragma unroll
    for (int w_ = 0; w_ < kTileWaves; ++w_) n_valid += sWaveCnt[w_];
    double *live = tile_cost + 2 * (size_t)n_tiles;
    const int row_first = run_id[blockIdx.x * kTile];
    const int rows_tile = run_id[blockIdx.x * kTile + tile_n - 1] - row_first + 1;
    if (n_valid == 0) {                                              // no active sample: the tile's rows are dead
        if (tid < rows_tile) live[row_first + tid] = 0.0;
        if (tid == 0) { tile_cost[2 * blockIdx.x] = 0.0; tile_cost[2 * blockIdx.x + 1] = 0.0; }
        return;
    }
    if (act) {                                                       // one Jacobian row per thread, at its compacted place
        sRow[pos] = (unsigned short)(run_id[s] - row_first);
        double Jrow[NJ];
        photo_row(node_dq, idx, w, K, p.lw.q, bh, nb, pf[0], pf[1], pf[2], g, sc, Jrow);
#pragma unroll
        for (int j = 0; j < NJ; ++j) sJ[pos * LD + j] = Jrow[j];
        sJ[pos * LD + NJ] = sc * r;
    }
    // the tile's objective, added in a fixed order; its count stays 0: cost_count[1] counts the data term's samples
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) obj += __shfl_xor(obj, o, 64);
    if (lane == 0) sObj[wv] = obj;
    __syncthreads();
    if (tid == 0) {
        double o = sObj[0];
#pragma unroll
        for (int w_ = 1; w_ < kTileWaves; ++w_) o += sObj[w_];
        tile_cost[2 * blockIdx.x] = o;
        tile_cost[2 * blockIdx.x + 1] = 0.0;
    }
    // run boundaries: sRun[0..n_runs] are the offsets in the compacted list where the scratch row changes
    {
        const bool head = tid < n_valid && (tid == 0 || sRow[tid] != sRow[tid - 1]);
        const unsigned long long hb = __ballot(head);
        if (lane == 0) sWaveCnt[wv] = __popcll(hb);       // (every thread passed the barrier after the first use)
        __syncthreads();
        int hp = __popcll(hb & ((1ull << lane) - 1ull));
        for (int w_ = 0; w_ < wv; ++w_) hp += sWaveCnt[w_];
        if (head) sRun[hp] = tid;
        if (tid == 0) {
            int n = 0;
            for (int w_ = 0; w_ < kTileWaves; ++w_) n += sWaveCnt[w_];
            sRun[n] = n_valid;
            sNRuns = n;
        }
        if (tid < rows_tile) sTouched[tid] = 0;
        __syncthreads();
    }
    const int n_runs = sNRuns;
    if (tid < n_runs) {
        partial[(size_t)(row_first + sRow[sRun[tid]]) * ST_ + NUP + NJ + 1] = (double)(sRun[tid + 1] - sRun[tid]);
        sTouched[sRow[sRun[tid]]] = 1;
    }
    __syncthreads();
    if (tid < rows_tile) live[row_first + tid] = sTouched[tid] ? 1.0 : 0.0;
    // Gram matrix of every run, G = X^T X with X = the run's rows of [J | r] (n x (6K + 1)), on the matrix cores as 16 x 16 tiles
    // of v_mfma_f64_16x16x4_f64 (gn_build_data_kernel's phase): one wave per run, runs dealt round-robin, rows in ascending sample
    // order, so the bits are the same every launch.
    constexpr int NC = NJ + 1;
    constexpr int NT = (NC + 15) / 16;
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int li = lane & 15, lk = lane >> 4;
    for (int rn = wv; rn < n_runs; rn += kTileWaves) {
        const int t0 = sRun[rn], t1 = sRun[rn + 1];
        d4 acc[NT * (NT + 1) / 2];
#pragma unroll
        for (int q = 0; q < NT * (NT + 1) / 2; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
        for (int t = t0; t < t1; t += 4) {
            double x[NT];                                            // A[i = li][k = lk] = B[k = lk][j = li] = X[t + lk][16 b + li]
#pragma unroll
            for (int b = 0; b < NT; ++b) {
                const int c = 16 * b + li;
                const double *src = sJ + (t + lk) * LD + c;
                x[b] = (t + lk < t1 && c < NC) ? *src : 0.0;
            }
            int q = 0;
#pragma unroll
            for (int bi = 0; bi < NT; ++bi)
#pragma unroll
                for (int bj = bi; bj < NT; ++bj, ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[bi], x[bj], acc[q], 0, 0, 0);
        }
        double *dst = partial + (size_t)(row_first + sRow[t0]) * ST_;
        int q = 0;
#pragma unroll
        for (int bi = 0; bi < NT; ++bi)
#pragma unroll
            for (int bj = bi; bj < NT; ++bj, ++q)
#pragma unroll
                for (int rr_ = 0; rr_ < 4; ++rr_) {                  // C/D: column = lane & 15, row = (lane >> 4) + 4 r
                    const int pa = 16 * bi + lk + 4 * rr_, pb = 16 * bj + li;
                    const double v = acc[q][rr_];
                    if (pa < NJ && pb < NJ) {
                        const int sa = pa / 6, sb = pb / 6;
                        if (sa <= sb) {
                            dst[36 * gn_sub(K, sa, sb) + 6 * (pa - 6 * sa) + (pb - 6 * sb)] = v;
                            // a diagonal sub-block that straddles two tiles: its lower entries lie in the tile that is not
                            // computed; the product is symmetric bit for bit
                            if (bi != bj && sa == sb) dst[36 * gn_sub(K, sa, sa) + 6 * (pb - 6 * sb) + (pa - 6 * sa)] = v;
                        }
                    } else if (pa < NJ && pb == NJ) {
                        dst[NUP + pa] = v;                           // J^T r
                    } else if (pa == NJ && pb == NJ) {
                        dst[NUP + NJ] = 0.5 * v;                     // sum of r^2, halved
                    }
                }
    }
}

int gn_add_photometric_impl(const dfh_gn_problem &q, const dfh_gn_frame &f, const dfh_gn_photometric &t, void *stream) {
    if (t.n == 0 || t.weight == 0.0) return DFH_OK;                  // nothing to add: no launch, the system stays as it is
    hipStream_t s = (hipStream_t)stream;
    const int n_tiles = (t.n + kTile - 1) / kTile;
    PhotoParams p;
    for (int i = 0; i < 9; ++i) { p.K.m[i] = f.K[i]; p.Kinv.m[i] = f.Kinv[i]; }
    for (int i = 0; i < 8; ++i) p.lw.q[i] = q.lw_dq[i];
    p.scale = f.scale; p.cx = f.center[0]; p.cy = f.center[1]; p.cz = f.center[2]; p.half = f.half;
    p.weight = t.weight; p.huber = t.huber_delta; p.max_diff = t.max_diff; p.band_sd = t.band_sd;
    p.H = f.H; p.W = f.W; p.n_views = f.n_views; p.depth_f64 = f.depth_dtype == DFH_F64 ? 1 : 0; p.n = t.n;
    p.views = static_cast<const AssocView *>(f.views);
    for (int v = 0; v < DFH_GN_MAX_VIEWS; ++v) p.color[v] = v < f.n_views ? static_cast<const unsigned *>(t.color[v]) : nullptr;
    double *tile_cost = t.partial + (size_t)t.n_rows * gn_row_stride(q.knn);      // 2 doubles per tile, then one live flag per row
    dim3 grid((unsigned)n_tiles), block(kTile);
#define DFH_PHOTO(KK)                                                                                                \
    case KK:                                                                                                         \
        hipLaunchKernelGGL(gn_photo_rows_kernel<KK>, grid, block, 0, s, t.pos, t.nbr, t.weights, t.ref, t.valid, t.conf, q.node_dq, p, \
                           t.run_id, t.partial, tile_cost, n_tiles, t.active_out, t.view_out, t.resid_out);          \
        break
    switch (q.knn) {
        DFH_PHOTO(1); DFH_PHOTO(2); DFH_PHOTO(3); DFH_PHOTO(4); DFH_PHOTO(5); DFH_PHOTO(6); DFH_PHOTO(7); DFH_PHOTO(8);
    }
#undef DFH_PHOTO
    DFH_HIP_CHECK(hipGetLastError());
    const int *upper = (q.blk_upper && q.n_upper > 0 && !on(opt().gn_gather_full)) ? q.blk_upper : nullptr;
    return gn_gather_launch(q.knn, t.partial, tile_cost + 2 * (size_t)n_tiles, t.n_rows, t.blk_ptr, t.blk_ent, q.n_blocks, t.node_ptr,
                            t.node_ent, q.n_nodes, q.vals, q.rhs, q.cost_count, tile_cost, n_tiles, true, upper, q.n_upper, stream);
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
