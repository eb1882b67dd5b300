// K21  camera tracking: the depth pyramid's halving step (dfh_depth_halve) and dense projective point-to-plane ICP of a frame's
// depth and normal maps against the model's predicted maps (dfh_icp_track).  No reference counterpart.  The semantics are
// written out operation by operation in include/dfusion_hip.h; tests/track_np.py restates them: the halved maps and the per-pixel
// rows agree bit for bit, the sums within their rounding bound, the solve bit for bit on the device's own sums.
//
// Shape of one ICP iteration, two launches:
//  rows   grid (kIcpGrid, V), 256 threads.  One lane per live pixel, a wave owns an 8 x 8-pixel tile (a workgroup 16 x 16), so
//         that the model-map gathers of a wave stay within a few lines.  Workgroup b walks the 16 x 16 tiles b, b + kIcpGrid, ..
//         of its view.  A wave writes sqrt(w) {J (6) | r | 0} of its 64 pixels to LDS and accumulates X^T X with
//         v_mfma_f64_16x16x4_f64, gn_global_rows_kernel's pattern: four accumulator doubles per lane hold all 28 sums (A's upper
//         triangle = entries (i <= j < 6), g = (i, 6), the objective = (6, 6)).  The workgroup publishes 29 partials.
//  finish grid (V), 1024 threads.  The kIcpGrid partial sets added in index order (32 chunks of consecutive sets, then the chunks),
//         the damped Cholesky solve, the guards and T <- exp(xi) T by one thread, the record to `stats`.
// kIcpGrid is a constant: the summation order does not follow the device, two runs give the same bits.  No float atomics, no
// private arrays (the solve's matrices live in LDS), nothing read back between iterations.
#include <cmath>

#include "dfh_common.h"

namespace dfh {

constexpr int kTrackMaxViews = 16;
constexpr int kIcpGrid = 256;           // workgroups per view of the rows kernel = partial sets per view
constexpr int kIcpVals = 29;            // 21 upper entries of A | 6 of g | objective | count
constexpr int kIcpRecord = 40;          // doubles per (view, iteration) record of `stats`

__device__ __forceinline__ bool track_valid(float d) { return d < 0.0f && d > -INFINITY; }

// ---- dfh_depth_halve ----------------------------------------------------------------------------------------------------
struct HalveArgs {
    const void *depth[kTrackMaxViews];
    int H, W, Ho, Wo;
    float J;
};

template <typename DepthT>
__global__ __launch_bounds__(256) void depth_halve_kernel(const HalveArgs a, float *__restrict__ out) {
    const int x = (int)blockIdx.x * 16 + (threadIdx.x & 15), y = (int)blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= a.Wo || y >= a.Ho) return;
    const DepthT *D = static_cast<const DepthT *>(a.depth[blockIdx.z]) + (size_t)(2 * y) * a.W + 2 * x;
    const float e0 = (float)D[0], e1 = (float)D[1], e2 = (float)D[a.W], e3 = (float)D[(size_t)a.W + 1];
    float sum = 0.0f, n = 0.0f;
    if (track_valid(e0)) {
        if (fabsf(e0 - e0) <= a.J) { sum = sum + e0; n = n + 1.0f; }
        if (track_valid(e1) && fabsf(e1 - e0) <= a.J) { sum = sum + e1; n = n + 1.0f; }
        if (track_valid(e2) && fabsf(e2 - e0) <= a.J) { sum = sum + e2; n = n + 1.0f; }
        if (track_valid(e3) && fabsf(e3 - e0) <= a.J) { sum = sum + e3; n = n + 1.0f; }
    }
    out[((size_t)blockIdx.z * a.Ho + y) * a.Wo + x] = n > 0.0f ? sum / n : 0.0f;
}

// ---- dfh_icp_track ------------------------------------------------------------------------------------------------------
struct IcpArgs {
    Mat3 K, Kinv;
    double max_dist2, min_cos2, huber;
    int H, W, ntx, n_tiles;
};

__global__ __launch_bounds__(256) void icp_rows_kernel(const float *__restrict__ Dl, const float *__restrict__ Nl, const float *__restrict__ Dm,
                                                        const float *__restrict__ Nm, const double *__restrict__ Tall, const IcpArgs a,
                                                        double *__restrict__ part, double *__restrict__ rows) {
    __shared__ double sPart[4][kIcpVals];
    __shared__ double sX[256 * 8];
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int view = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const double *T = Tall + 12 * (size_t)view;
    const double T00 = T[0], T01 = T[1], T02 = T[2], T03 = T[3], T10 = T[4], T11 = T[5], T12 = T[6], T13 = T[7], T20 = T[8], T21 = T[9],
                 T22 = T[10], T23 = T[11];
    const size_t vbase = (size_t)view * a.H * a.W;
    d4 acc = d4{0.0, 0.0, 0.0, 0.0};
    double cnt = 0.0;
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += kIcpGrid) {
        const int x = (tile % a.ntx) * 16 + (wv & 1) * 8 + (lane & 7);
        const int y = (tile / a.ntx) * 16 + (wv >> 1) * 8 + (lane >> 3);
        const bool inside = x < a.W && y < a.H;
        const size_t pix = vbase + (size_t)(inside ? y : 0) * a.W + (inside ? x : 0);
        double J0 = 0.0, J1 = 0.0, J2 = 0.0, J3 = 0.0, J4 = 0.0, J5 = 0.0, r = 0.0, w = 0.0;
        bool ok = inside;
        // 1. live validity
        const float df = Dl[pix];
        ok = ok && track_valid(df);
        double l0 = 0.0, l1 = 0.0, l2 = 0.0;
        if (Nl) {
            l0 = (double)Nl[3 * pix]; l1 = (double)Nl[3 * pix + 1]; l2 = (double)Nl[3 * pix + 2];
            const double ll = (l0 * l0 + l1 * l1) + l2 * l2;
            ok = ok && ll > 0.0;
        }
        // 2. live vertex
        const double d = (double)df, X = (double)x, Y = (double)y;
        const double rho0 = (a.Kinv.m[0] * X + a.Kinv.m[1] * Y) + a.Kinv.m[2];
        const double rho1 = (a.Kinv.m[3] * X + a.Kinv.m[4] * Y) + a.Kinv.m[5];
        const double rho2 = (a.Kinv.m[6] * X + a.Kinv.m[7] * Y) + a.Kinv.m[8];
        const double V0 = (-d) * rho0, V1 = (-d) * rho1, V2 = (-d) * rho2;
        const double P0 = ((T00 * V0 + T01 * V1) + T02 * V2) + T03;
        const double P1 = ((T10 * V0 + T11 * V1) + T12 * V2) + T13;
        const double P2 = ((T20 * V0 + T21 * V1) + T22 * V2) + T23;
        // 3. projection
        const double q0 = (a.K.m[0] * P0 + a.K.m[1] * P1) + a.K.m[2] * P2;
        const double q1 = (a.K.m[3] * P0 + a.K.m[4] * P1) + a.K.m[5] * P2;
        const double q2 = (a.K.m[6] * P0 + a.K.m[7] * P1) + a.K.m[8] * P2;
        ok = ok && q2 > 0.0 && q2 < __builtin_huge_val();
        const double ui = rint(q0 / q2), vi = rint(q1 / q2);
        ok = ok && ui >= 0.0 && ui <= (double)(a.W - 1) && vi >= 0.0 && vi <= (double)(a.H - 1);
        if (ok) {
            // 4. model side
            const size_t mp = vbase + (size_t)(int)vi * a.W + (size_t)(int)ui;
            const float mf = Dm[mp];
            const double n0 = (double)Nm[3 * mp], n1 = (double)Nm[3 * mp + 1], n2 = (double)Nm[3 * mp + 2];
            const double nn = (n0 * n0 + n1 * n1) + n2 * n2;
            ok = track_valid(mf) && nn > 0.0;
            const double m = (double)mf;
            const double s0 = (a.Kinv.m[0] * ui + a.Kinv.m[1] * vi) + a.Kinv.m[2];
            const double s1 = (a.Kinv.m[3] * ui + a.Kinv.m[4] * vi) + a.Kinv.m[5];
            const double s2 = (a.Kinv.m[6] * ui + a.Kinv.m[7] * vi) + a.Kinv.m[8];
            const double M0 = (-m) * s0, M1 = (-m) * s1, M2 = (-m) * s2;
            // 5. gates
            const double e0 = P0 - M0, e1 = P1 - M1, e2 = P2 - M2;
            const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
            if (a.max_dist2 > 0.0) ok = ok && d2 <= a.max_dist2;
            if (Nl) {
                const double R0 = (T00 * l0 + T01 * l1) + T02 * l2;
                const double R1 = (T10 * l0 + T11 * l1) + T12 * l2;
                const double R2 = (T20 * l0 + T21 * l1) + T22 * l2;
                const double c = (R0 * n0 + R1 * n1) + R2 * n2;
                const double mm = (R0 * R0 + R1 * R1) + R2 * R2;
                ok = ok && c > 0.0 && c * c >= a.min_cos2 * (mm * nn);
            }
            if (ok) {
                // 6. row
                r = (n0 * e0 + n1 * e1) + n2 * e2;
                J0 = P1 * n2 - P2 * n1;
                J1 = P2 * n0 - P0 * n2;
                J2 = P0 * n1 - P1 * n0;
                J3 = n0; J4 = n1; J5 = n2;
                w = 1.0;
                if (a.huber > 0.0 && fabs(r) > a.huber) w = a.huber / fabs(r);
                cnt += 1.0;
            }
        }
        if (rows && inside) {
            double *o = rows + 8 * pix;
            o[0] = J0; o[1] = J1; o[2] = J2; o[3] = J3; o[4] = J4; o[5] = J5; o[6] = r; o[7] = w;
        }
        const double sc = sqrt(w);
        double *row = sX + 8 * tid;
        row[0] = sc * J0; row[1] = sc * J1; row[2] = sc * J2; row[3] = sc * J3; row[4] = sc * J4; row[5] = sc * J5;
        row[6] = sc * r; row[7] = 0.0;
        // (a wave reads only the rows its own lanes wrote; its LDS operations execute in order: no workgroup barrier)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
#pragma unroll 4
        for (int st = 0; st < 16; ++st) {                                     // A[i = li][k = lk] = B[k = lk][j = li] = X[64 wv + 4 st + lk][li]
            const double xv = li < 8 ? sX[8 * (64 * wv + 4 * st + lk) + li] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xv, xv, acc, 0, 0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {                                          // C/D: column = lane & 15, row = (lane >> 4) + 4 r
        const int pa = lk + 4 * r4, pb = li;
        if (pa < 6 && pb >= pa && pb < 6) sPart[wv][pa * 6 - (pa * (pa - 1)) / 2 + (pb - pa)] = acc[r4];
        else if (pa < 6 && pb == 6) sPart[wv][21 + pa] = acc[r4];
        else if (pa == 6 && pb == 6) sPart[wv][27] = acc[r4];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) sPart[wv][28] = cnt;
    __syncthreads();
    if (tid < kIcpVals)
        part[((size_t)view * kIcpGrid + blockIdx.x) * kIcpVals + tid] = ((sPart[0][tid] + sPart[1][tid]) + sPart[2][tid]) + sPart[3][tid];
}

struct IcpFinishArgs {
    double lm_rel, min_count, max_rot2, max_trans2;
    int n_iters, iter;
};

__global__ __launch_bounds__(1024) void icp_finish_kernel(const double *__restrict__ part, const IcpFinishArgs f, double *__restrict__ Tall,
                                                           double *__restrict__ stats) {
    __shared__ double chunk_sum[32][32];
    __shared__ double sv[32];
    __shared__ double sL[36], sy[6], sxi[6], sR[9], sVm[9], sT[12];
    const int view = blockIdx.x;
    const int e = threadIdx.x & 31, chunk = threadIdx.x >> 5;
    constexpr int per = kIcpGrid / 32;
    const double *p = part + (size_t)view * kIcpGrid * kIcpVals;
    double v = 0.0;
    if (e < kIcpVals) {
        double xs[per];
#pragma unroll
        for (int j = 0; j < per; ++j) xs[j] = p[(size_t)(chunk * per + j) * kIcpVals + e];
#pragma unroll
        for (int j = 0; j < per; ++j) v += xs[j];
    }
    chunk_sum[chunk][e] = v;
    __syncthreads();
    double *rec = stats + ((size_t)view * f.n_iters + f.iter) * kIcpRecord;
    if (threadIdx.x < kIcpVals) {
        double s = chunk_sum[0][threadIdx.x];
#pragma unroll
        for (int c = 1; c < 32; ++c) s += chunk_sum[c][threadIdx.x];
        sv[threadIdx.x] = s;
        rec[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double *T = Tall + 12 * (size_t)view;
    bool step = sv[28] >= f.min_count;
    for (int i = 0; i < 6; ++i) sxi[i] = 0.0;
    if (step) {
        // D = A + lm_rel diag A, factored in place: L's column j after columns < j
        for (int j = 0; j < 6 && step; ++j) {
            const int qjj = j * 6 - (j * (j - 1)) / 2;
            double s = sv[qjj] + f.lm_rel * sv[qjj];
            for (int k = 0; k < j; ++k) s = s - sL[6 * j + k] * sL[6 * j + k];
            if (!(s > 0.0 && s < __builtin_huge_val())) { step = false; break; }
            const double ljj = sqrt(s);
            sL[7 * j] = ljj;
            for (int i = j + 1; i < 6; ++i) {
                double t = sv[qjj + (i - j)];
                for (int k = 0; k < j; ++k) t = t - sL[6 * i + k] * sL[6 * j + k];
                sL[6 * i + j] = t / ljj;
            }
        }
    }
    if (step) {
        for (int i = 0; i < 6; ++i) {                                        // L y = -g
            double t = -sv[21 + i];
            for (int k = 0; k < i; ++k) t = t - sL[6 * i + k] * sy[k];
            sy[i] = t / sL[7 * i];
        }
        for (int i = 5; i >= 0; --i) {                                       // L^T xi = y
            double t = sy[i];
            for (int k = i + 1; k < 6; ++k) t = t - sL[6 * k + i] * sxi[k];
            sxi[i] = t / sL[7 * i];
        }
        const double ww = (sxi[0] * sxi[0] + sxi[1] * sxi[1]) + sxi[2] * sxi[2];
        const double vv = (sxi[3] * sxi[3] + sxi[4] * sxi[4]) + sxi[5] * sxi[5];
        step = ww <= f.max_rot2 && vv <= f.max_trans2;                        // (a NaN refuses)
        if (step) {
            const double o0 = sxi[0], o1 = sxi[1], o2 = sxi[2];
            double ca, cb, cc;
            if (ww < 1e-8) {
                ca = 1.0 - ww / 6.0;
                cb = 0.5 - ww / 24.0;
                cc = 1.0 / 6.0 - ww / 120.0;
            } else {
                const double th = sqrt(ww);
                const double sn = sin(th), cs = cos(th);
                ca = sn / th;
                cb = (1.0 - cs) / ww;
                cc = (th - sn) / (ww * th);
            }
            // Omega = [w]x, Omega^2 = w w^T - ww I
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    const double oi = i == 0 ? o0 : (i == 1 ? o1 : o2), oj = j == 0 ? o0 : (j == 1 ? o1 : o2);
                    const double eye = i == j ? 1.0 : 0.0;
                    double om = 0.0;
                    if (i == 0 && j == 1) om = -o2; else if (i == 0 && j == 2) om = o1; else if (i == 1 && j == 0) om = o2;
                    else if (i == 1 && j == 2) om = -o0; else if (i == 2 && j == 0) om = -o1; else if (i == 2 && j == 1) om = o0;
                    const double om2 = i == j ? oi * oj - ww : oi * oj;
                    sR[3 * i + j] = (eye + ca * om) + cb * om2;
                    sVm[3 * i + j] = (eye + cb * om) + cc * om2;
                }
            for (int rr = 0; rr < 3; ++rr) {
                const double t = (sVm[3 * rr] * sxi[3] + sVm[3 * rr + 1] * sxi[4]) + sVm[3 * rr + 2] * sxi[5];
                for (int c = 0; c < 4; ++c) {
                    const double m = (sR[3 * rr] * T[c] + sR[3 * rr + 1] * T[4 + c]) + sR[3 * rr + 2] * T[8 + c];
                    sT[4 * rr + c] = c == 3 ? m + t : m;
                }
            }
            for (int i = 0; i < 12; ++i) T[i] = sT[i];
        }
    }
    rec[29] = step ? 1.0 : 0.0;
    for (int i = 0; i < 6; ++i) rec[30 + i] = step ? sxi[i] : 0.0;
    for (int i = 36; i < kIcpRecord; ++i) rec[i] = 0.0;
}

}  // namespace dfh

// =================================================================================== C ABI
extern "C" int dfh_depth_halve(const void *const *depth, int n_views, int depth_dtype, int H, int W, double max_jump, float *out,
                               void *stream) {
    using namespace dfh;
    static const char *const me = "dfh_depth_halve";
    DFH_REQUIRE(depth && out, "%s: null depth array or output", me);
    DFH_REQUIRE(n_views >= 1 && n_views <= kTrackMaxViews, "%s: %d views (1..%d per call)", me, n_views, kTrackMaxViews);
    DFH_REQUIRE(depth_dtype == DFH_F32 || depth_dtype == DFH_F64, "%s: bad depth dtype %d", me, depth_dtype);
    DFH_REQUIRE(H >= 2 && W >= 2 && (long)H * W < (1L << 31), "%s: bad image size %dx%d", me, H, W);
    DFH_REQUIRE(std::isfinite(max_jump) && max_jump >= 0.0, "%s: max_jump %g is not finite and >= 0", me, max_jump);
    HalveArgs a = {};
    for (int v = 0; v < n_views; ++v) {
        DFH_REQUIRE(depth[v], "%s: null depth map %d", me, v);
        DFH_REQUIRE(depth[v] != (const void *)out, "%s: the output aliases depth map %d", me, v);
        a.depth[v] = depth[v];
    }
    a.H = H; a.W = W; a.Ho = H / 2; a.Wo = W / 2;
    a.J = (float)max_jump;
    DFH_REQUIRE((a.Ho + 15) / 16 <= 65535, "%s: image too tall", me);
    const dim3 grid((unsigned)((a.Wo + 15) / 16), (unsigned)((a.Ho + 15) / 16), (unsigned)n_views);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (depth_dtype == DFH_F64) hipLaunchKernelGGL(depth_halve_kernel<double>, grid, dim3(256), 0, s, a, out);
    else hipLaunchKernelGGL(depth_halve_kernel<float>, grid, dim3(256), 0, s, a, out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

extern "C" size_t dfh_icp_track_bytes(int n_views) {
    if (n_views < 1 || n_views > dfh::kTrackMaxViews) return 0;
    return sizeof(double) * (size_t)n_views * dfh::kIcpGrid * dfh::kIcpVals;
}

extern "C" int dfh_icp_track(const dfh_icp_track_params *p, void *stream) {
    using namespace dfh;
    static const char *const me = "dfh_icp_track";
    DFH_REQUIRE(p, "%s: null params", me);
    DFH_REQUIRE(p->n_views >= 1 && p->n_views <= kTrackMaxViews, "%s: %d views (1..%d per call)", me, p->n_views, kTrackMaxViews);
    DFH_REQUIRE(p->H >= 1 && p->W >= 1 && (long)p->H * p->W < (1L << 31), "%s: bad image size %dx%d", me, p->H, p->W);
    DFH_REQUIRE(p->live_depth && p->model_depth && p->model_normals, "%s: null live_depth, model_depth or model_normals", me);
    DFH_REQUIRE(p->n_iters >= 0 && p->n_iters <= 64, "%s: n_iters=%d outside [0,64]", me, p->n_iters);
    DFH_REQUIRE(p->T && p->scratch && (p->stats || p->n_iters == 0), "%s: null T, stats or scratch", me);
    for (int i = 0; i < 9; ++i)
        DFH_REQUIRE(std::isfinite(p->K[i]) && std::isfinite(p->Kinv[i]), "%s: K or Kinv is not finite", me);
    DFH_REQUIRE(std::isfinite(p->max_dist) && p->max_dist >= 0.0, "%s: max_dist %g is not finite and >= 0", me, p->max_dist);
    DFH_REQUIRE(p->min_cos >= 0.0 && p->min_cos <= 1.0, "%s: min_cos %g outside [0,1]", me, p->min_cos);
    DFH_REQUIRE(std::isfinite(p->huber) && p->huber >= 0.0, "%s: huber %g is not finite and >= 0", me, p->huber);
    DFH_REQUIRE(std::isfinite(p->lm_rel) && p->lm_rel >= 0.0, "%s: lm_rel %g is not finite and >= 0", me, p->lm_rel);
    DFH_REQUIRE(p->min_count >= 6, "%s: min_count=%d below 6", me, p->min_count);
    DFH_REQUIRE(p->max_rot > 0.0 && p->max_trans > 0.0, "%s: max_rot and max_trans must be > 0", me);     // (NaN fails, +inf passes)
    DFH_REQUIRE(p->scratch_bytes >= dfh_icp_track_bytes(p->n_views), "%s: scratch too small (need %zu bytes)", me,
                dfh_icp_track_bytes(p->n_views));
    if (p->n_iters == 0) return DFH_OK;
    IcpArgs a = {};
    for (int i = 0; i < 9; ++i) { a.K.m[i] = p->K[i]; a.Kinv.m[i] = p->Kinv[i]; }
    a.max_dist2 = p->max_dist * p->max_dist;
    a.min_cos2 = p->min_cos * p->min_cos;
    a.huber = p->huber;
    a.H = p->H; a.W = p->W;
    a.ntx = (p->W + 15) / 16;
    const long n_tiles = (long)a.ntx * ((p->H + 15) / 16);
    DFH_REQUIRE(n_tiles < (1L << 31) - kIcpGrid, "%s: too many tiles", me);
    a.n_tiles = (int)n_tiles;
    IcpFinishArgs f = {};
    f.lm_rel = p->lm_rel; f.min_count = (double)p->min_count;
    f.max_rot2 = p->max_rot * p->max_rot; f.max_trans2 = p->max_trans * p->max_trans;
    f.n_iters = p->n_iters;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *part = static_cast<double *>(p->scratch);
    for (int it = 0; it < p->n_iters; ++it) {
        f.iter = it;
        hipLaunchKernelGGL(icp_rows_kernel, dim3(kIcpGrid, (unsigned)p->n_views), dim3(256), 0, s, p->live_depth, p->live_normals,
                           p->model_depth, p->model_normals, (const double *)p->T, a, part, it == 0 ? p->rows : nullptr);
        hipLaunchKernelGGL(icp_finish_kernel, dim3((unsigned)p->n_views), dim3(1024), 0, s, (const double *)part, f, p->T, p->stats);
    }
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}
