// The rigid mode of the warp-field solve: ONE twist shared by all nodes, which ten block-Jacobi PCG iterations barely move.
// From the assembled block system (dfh_gn_global_step) or from a subsample of the data rows without building it
// (dfh_gn_global_sampled; its rows are associated and differentiated by dfh_gn_rows.h exactly as in the build), the twist
// decay between frames (dfh_relax_twists), and the packing of the symmetric system for the exchange between ranks.
// Restated in oracle/gn_np.py (global_step, global_step_sampled, relax_twists).
#include "dfh_assoc_volume.h"
#include "dfh_gn_rows.h"

#include <algorithm>
#include <type_traits>

namespace dfh {

// dq <- exp(factor * log(dq)): the node's rotation vector and translation both scaled by factor in [0, 1] -- a decoupled scaling of
// the two, not a scaling along the motion's screw.  log of a dual quaternion (q | qe) with q = |q| (cos(t/2), sin(t/2) n):
// omega = t n, v = 2 vec(qe q*) / |q|^2 -- the inverse of apply_twist_one's exp for a unit q; a non-unit q (the solve never
// renormalises) comes back unit.  q and -q are the same motion: the DQ is taken with w >= 0 (v is bilinear in (q, qe): the sign
// cancels there), so t is in [0, pi] -- with w < 0 the angle would be 2 pi - t the other way round, and scaling it a different
// rotation.  Restated in oracle/gn_np.relax_twists.
__global__ __launch_bounds__(256) void relax_twist_kernel(double *__restrict__ node_dq, int N, double factor) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= N) return;
    double *d = node_dq + 8 * (size_t)a;
    const double sg = d[0] < 0.0 ? -1.0 : 1.0;
    const double w = sg * d[0], x = sg * d[1], y = sg * d[2], z = sg * d[3];
    const double n2 = (w * w + x * x) + (y * y + z * z);
    if (!(n2 > 1e-300) || !(n2 < 1e300)) return;                               // (zero / non-finite: left alone)
    const double vn = sqrt(x * x + y * y + z * z);
    const double th = 2.0 * atan2(vn, w);                                      // rotation angle, [0, pi]
    const double k = vn > 1e-12 ? th / vn : 2.0 / sqrt(n2);                    // omega = k (x, y, z)
    // (0, v) = 2 qe q* / |q|^2
    const double e0 = sg * d[4], e1 = sg * d[5], e2 = sg * d[6], e3 = sg * d[7];
    const double inv = 2.0 / n2;
    const double vx = inv * (-e0 * x + e1 * w - e2 * z + e3 * y);
    const double vy = inv * (-e0 * y + e2 * w - e3 * x + e1 * z);
    const double vz = inv * (-e0 * z + e3 * w - e1 * y + e2 * x);
    d[0] = 1.0; d[1] = d[2] = d[3] = d[4] = d[5] = d[6] = d[7] = 0.0;
    apply_twist_one(d, factor * k * x, factor * k * y, factor * k * z, factor * vx, factor * vy, factor * vz);
}

// ---- the rigid mode of the normal equations (round 4) ------------------------------------------------------------
// Ten block-Jacobi PCG iterations barely move the smoothest mode of the system -- all nodes moving together -- which the
// regulariser does not penalise and the preconditioner does not see: of a pure 0.6-voxel translation the shipped ten GN
// iterations recover 28 % along the normals, the exactly solved loop 70 % (tests/golden/solve_recovery.json).  The coarse
// correction: restrict the system to ONE twist shared by all nodes, x_a = xi for every a -- A_g = sum of all 6x6 blocks,
// g_g = sum of all J^T r -- solve (A_g + lm diag A_g) xi = -g_g and apply xi to every node.  kGlobalWgs workgroups add their
// share of the blocks (wave w of the grid: blocks w, w + n_waves, ...; lane e < 36 one matrix entry, lanes 36..41 the J^T r
// entries of nodes w, w + n_waves, ...), publish 42 partial sums, and the workgroup that draws the last ticket adds the
// partials in index order (same bits every run), solves by Cholesky and applies the twist.
constexpr int kGlobalWgs = 64;
__global__ __launch_bounds__(256) void gn_global_step_kernel(const double *__restrict__ vals, int n_blocks, const double *__restrict__ rhs, int N,
                                                              double lm_rel, double *__restrict__ node_dq, double *__restrict__ xi_out,
                                                              double *__restrict__ scratch /* kGlobalWgs x 42 partials | ticket */) {
    __shared__ double part[4][42];
    __shared__ double sA[36], sg[6], sxi[6];
    __shared__ unsigned s_ticket;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wave = blockIdx.x * 4 + wv, n_waves = gridDim.x * 4;
    double acc = 0.0;
    if (lane < 36) {
        for (int b = wave; b < n_blocks; b += n_waves) acc += vals[36 * (size_t)b + lane];
    } else if (lane < 42) {
        for (int a = wave; a < N; a += n_waves) acc += rhs[6 * (size_t)a + (lane - 36)];
    }
    if (lane < 42) part[wv][lane] = acc;
    __syncthreads();
    if (threadIdx.x < 42)
        __hip_atomic_store(scratch + 42 * (size_t)blockIdx.x + threadIdx.x,
                           ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    unsigned *ticket = reinterpret_cast<unsigned *>(scratch + 42 * (size_t)gridDim.x);
    if (threadIdx.x == 0) s_ticket = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_ticket != gridDim.x - 1) return;
    if (threadIdx.x < 42) {
        double v = 0.0;
        for (unsigned w = 0; w < gridDim.x; ++w) v += __hip_atomic_load(scratch + 42 * (size_t)w + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (threadIdx.x < 36) sA[threadIdx.x] = v; else sg[threadIdx.x - 36] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double D[36];
#pragma unroll
        for (int e = 0; e < 36; ++e) D[e] = 0.5 * (sA[e] + sA[6 * (e % 6) + e / 6]);        // (symmetric up to summation order: symmetrised)
#pragma unroll
        for (int d = 0; d < 6; ++d) D[7 * d] = D[7 * d] + lm_rel * D[7 * d];
        double row[6];
        inv6_row(D, (int)threadIdx.x, row);
        double x = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) x -= row[j] * sg[j];
        const bool ok = fabs(x) < 1e6;                                                       // (NaN / a singular system: no step)
        sxi[threadIdx.x] = ok ? x : 0.0;
    }
    __syncthreads();
    if (threadIdx.x < 6 && xi_out) xi_out[threadIdx.x] = sxi[threadIdx.x];
    if (threadIdx.x == 0) *ticket = 0u;                                                      // (ready for the next call)
    bool all_ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) all_ok = all_ok && sxi[j] == sxi[j];
    if (!all_ok) return;
    for (int a = threadIdx.x; a < N; a += 256) apply_twist_one(node_dq + 8 * (size_t)a, sxi[0], sxi[1], sxi[2], sxi[3], sxi[4], sxi[5]);
}

// The rigid mode from a SUBSAMPLE of the data rows, without building the block system (round 4): for a twist shared by all
// nodes a sample's Jacobian is the sum of its k node blocks, J_g = sum_a J_a (6 entries), so A_g = sum_s J_g^T J_g and
// g_g = sum_s J_g^T r need neither runs nor a gather.  Every `stride`-th 128-sample tile (the samples are sorted by node tuple:
// a uniform thinning of the surface) is associated and differentiated exactly as in gn_build_data_kernel (same Huber weights);
// the regulariser is left out (a common left twist rotates every regulariser residual rigidly: it only damps this mode).  Per
// tile 21 + 6 sums (+ objective, count) in a fixed order; gn_global_finish_kernel adds the workgroups' partials in index order,
// damps, solves and applies the twist to every node (sharded samples: it stops at the 29 sums, an all-reduce goes in between and
// gn_global_apply_kernel does the rest).  Restated in oracle/gn_np.global_step_sampled.
constexpr int kGlobalVals = 29;                     // 21 upper entries of A_g | 6 of g_g | objective | valid count
constexpr int kGlobalGrid = 1536;                   // workgroups of the rows kernel = partial sets (fixed: the summation order must not follow the device)
// The sums on the matrix cores, like the data rows' Gram matrices: a wave writes {J_g (6) | r | 0} of its 64 samples to LDS and
// accumulates X^T X with v_mfma_f64_16x16x4 (16 steps of four samples per tile; A_g and g_g are its entries (i <= j < 6) and
// (i, 6)); the accumulator is four doubles per lane where 27 running sums per thread made the kernel a 256-VGPR one: one wave
// per SIMD, a tile's whole chain of dependent loads exposed -- 65 us for config 3's 762 tiles, 131 us for config 5's 5.2 k.
// VOLUME: the samples are associated against a live TSDF volume of DepthT (one trilinear cell, dfh_assoc_volume.h) instead of
// the frame's views; the kernel's last argument is what its association reads.  GATED: the views through the normal gate
// (associate_views<.., true>): the sample's warped normal is computed in front of the association, the gate's arguments travel in
// this mode's own struct.
template <int K, typename DepthT, bool VOLUME = false, bool GATED = false>
__global__ __launch_bounds__(kTile) __attribute__((amdgpu_waves_per_eu(3, 8))) void gn_global_rows_kernel(const double *__restrict__ spos, const double *__restrict__ snrm,
                                                              const int *__restrict__ nbr, const double *__restrict__ wts,
                                                              const double *__restrict__ node_dq, const BuildParams p, int stride, long n_sub,
                                                              double *__restrict__ tile_part,
                                                              const std::conditional_t<VOLUME, VolAssocArgs, std::conditional_t<GATED, GatedAssocArgs, AssocArgs>> aa) {
    static_assert(!(VOLUME && GATED), "the normal gate is the depth term's");
    __shared__ double sPart[kTileWaves][kGlobalVals];
    __shared__ double sX[kTile * 8];
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    d4 acc = d4{0.0, 0.0, 0.0, 0.0};
    double obj_acc = 0.0, cnt_acc = 0.0;
    // a workgroup walks the tiles blockIdx.x, + gridDim.x, ... of the thinned list and keeps its sums: at most kGlobalGrid
    // partial sets for the finish kernel (one set per TILE made that kernel's serial adds the whole step: 1.3 ms)
    for (long sub = blockIdx.x; sub < n_sub; sub += gridDim.x) {
        const long s = sub * stride * kTile + tid;
        double jg[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, rr = 0.0;
        if (s < p.S) {
            int idx[kKMaxS];
            double w[kKMaxS];
#pragma unroll
            for (int j = 0; j < kKMaxS; ++j) {
                idx[j] = j < K ? nbr[(size_t)s * K + j] : 0;
                w[j] = j < K ? wts[(size_t)s * K + j] : 0.0;
            }
            double bh[8];
            const double nb = blend_static(node_dq, idx, w, K, bh);
            const double pfx = round_f32(spos[3 * (size_t)s]), pfy = round_f32(spos[3 * (size_t)s + 1]), pfz = round_f32(spos[3 * (size_t)s + 2]);
            const D3 x1 = dqb_warp_exact(bh, pfx, pfy, pfz);
            const D3 xp = dqb_warp_exact(p.lw.q, round_f32(x1.x), round_f32(x1.y), round_f32(x1.z));
            double c[3];
            bool ok;                                                              // (a lane with s >= S is not here: it touches no map, no volume)
            if constexpr (VOLUME) ok = associate_volume_cell<DepthT>(static_cast<const DepthT *>(aa.live), aa.vp, xp, c);
            else if constexpr (GATED) {
                const D3 np_ = warped_normal(bh, p.lw.q, snrm[3 * (size_t)s], snrm[3 * (size_t)s + 1], snrm[3 * (size_t)s + 2]);
                ok = associate_views<DepthT, true>(aa.ap, aa.views, aa.n_views, xp, c, ~0u, aa.ng.normals, aa.ng.min_cos, np_.x, np_.y, np_.z);
            } else ok = associate_views<DepthT>(aa.ap, aa.views, aa.n_views, xp, c);
            if (ok) {
                double Jrow[6 * K];
                double r = data_row_from(node_dq, idx, w, K, p.lw.q, bh, nb, pfx, pfy, pfz, xp, snrm[3 * (size_t)s], snrm[3 * (size_t)s + 1],
                                         snrm[3 * (size_t)s + 2], c[0], c[1], c[2], Jrow);
                double obj = 0.5 * r * r, sc = 1.0;
                if (p.huber > 0.0 && fabs(r) > p.huber) {
                    obj = p.huber * (fabs(r) - 0.5 * p.huber);
                    sc = sqrt(p.huber / fabs(r));
                }
                rr = r * sc;
#pragma unroll
                for (int c6 = 0; c6 < 6; ++c6) {
                    double v = 0.0;
#pragma unroll
                    for (int a = 0; a < K; ++a) v += Jrow[6 * a + c6];
                    jg[c6] = v * sc;
                }
                obj_acc += obj;
                cnt_acc += 1.0;
            }
        }
        double *row = sX + 8 * tid;
#pragma unroll
        for (int c6 = 0; c6 < 6; ++c6) row[c6] = jg[c6];
        row[6] = rr; row[7] = 0.0;
        // (a wave reads only the rows its own lanes wrote; its LDS operations execute in order: no workgroup barrier)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
#pragma unroll 4
        for (int st = 0; st < 16; ++st) {                                     // A[i = li][k = lk] = B[k = lk][j = li] = X[64 wv + 4 st + lk][li]
            const double x = li < 8 ? sX[8 * (64 * wv + 4 * st + lk) + li] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, acc, 0, 0, 0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {                                          // C/D: column = lane & 15, row = (lane >> 4) + 4 r
        const int pa = lk + 4 * r4, pb = li;
        if (pa < 6 && pb >= pa && pb < 6) sPart[wv][pa * 6 - (pa * (pa - 1)) / 2 + (pb - pa)] = acc[r4];
        else if (pa < 6 && pb == 6) sPart[wv][21 + pa] = acc[r4];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { obj_acc += __shfl_xor(obj_acc, o, 64); cnt_acc += __shfl_xor(cnt_acc, o, 64); }
    if (lane == 0) { sPart[wv][27] = obj_acc; sPart[wv][28] = cnt_acc; }
    __syncthreads();
    if (tid < kGlobalVals) {
        double v = sPart[0][tid];
#pragma unroll
        for (int w_ = 1; w_ < kTileWaves; ++w_) v += sPart[w_][tid];
        tile_part[(size_t)blockIdx.x * kGlobalVals + tid] = v;
    }
}

// the damped 6 x 6 solve and the twist for every node, from the 29 sums in LDS (sv); sxi: scratch
__device__ __forceinline__ void global_solve_apply(const double *sv, double *sxi, double lm_rel, int N, double *__restrict__ node_dq,
                                                   double *__restrict__ xi_out) {
    if (threadIdx.x < 6) {
        double D[36];
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) { D[6 * i + j] = sv[q]; D[6 * j + i] = sv[q]; ++q; }
#pragma unroll
        for (int d = 0; d < 6; ++d) D[7 * d] = D[7 * d] + lm_rel * D[7 * d];
        double row[6];
        inv6_row(D, (int)threadIdx.x, row);
        double x = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) x -= row[j] * sv[21 + j];
        sxi[threadIdx.x] = (fabs(x) < 1e6 && sv[28] >= 6.0) ? x : 0.0;             // (NaN, a singular system, hardly any data: no step)
    }
    __syncthreads();
    if (xi_out) {
        if (threadIdx.x < 6) xi_out[threadIdx.x] = sxi[threadIdx.x];
        if (threadIdx.x == 6) xi_out[6] = sv[27];
        if (threadIdx.x == 7) xi_out[7] = sv[28];
    }
    for (int a = threadIdx.x; a < N; a += blockDim.x) apply_twist_one(node_dq + 8 * (size_t)a, sxi[0], sxi[1], sxi[2], sxi[3], sxi[4], sxi[5]);
}

// the workgroups' partials added in index order (32 chunks of consecutive sets, sixteen loads in flight per thread, then the
// chunks): 29 sums; APPLY: the solve and the twists in the same launch (one rank: nothing to all-reduce in between).  The old
// pair -- 8 chunks of 128 dependent load-and-add steps, then a launch for the solve -- took 29 + 8 us.
template <bool APPLY>
__global__ __launch_bounds__(1024) void gn_global_finish_kernel(const double *__restrict__ tile_part, int n_sets, double *__restrict__ sums,
                                                                 double lm_rel, int N, double *__restrict__ node_dq, double *__restrict__ xi_out) {
    __shared__ double part[32][32];
    __shared__ double sv[32], sxi[6];
    const int e = threadIdx.x & 31, chunk = threadIdx.x >> 5;
    const int per = (n_sets + 31) / 32;
    const int t0 = chunk * per, t1 = min(n_sets, t0 + per);
    double v = 0.0;
    for (int t = t0; t < t1; t += 16) {
        double x[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) x[j] = (t + j < t1 && e < kGlobalVals) ? tile_part[(size_t)(t + j) * kGlobalVals + e] : 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) v += x[j];
    }
    part[chunk][e] = v;
    __syncthreads();
    if (threadIdx.x < kGlobalVals) {
        double a = part[0][threadIdx.x];
#pragma unroll
        for (int c = 1; c < 32; ++c) a += part[c][threadIdx.x];
        sv[threadIdx.x] = a;
        sums[threadIdx.x] = a;
    }
    __syncthreads();
    if (APPLY) global_solve_apply(sv, sxi, lm_rel, N, node_dq, xi_out);
}

// (A_g + lm diag A_g) xi = -g_g from the 29 sums (after an all-reduce over ranks, where the samples are sharded), xi to every node
__global__ __launch_bounds__(256) void gn_global_apply_kernel(const double *__restrict__ sums, double lm_rel, int N, double *__restrict__ node_dq,
                                                               double *__restrict__ xi_out /* 6 | objective, count */) {
    __shared__ double sv[kGlobalVals], sxi[6];
    if (threadIdx.x < kGlobalVals) sv[threadIdx.x] = sums[threadIdx.x];
    __syncthreads();
    global_solve_apply(sv, sxi, lm_rel, N, node_dq, xi_out);
}

}  // namespace dfh

// =================================================================================== C ABI
extern "C" {

// J^T J is symmetric: block (b, a) is the transpose of block (a, b).  Between ranks only the blocks with col >= row travel
// (about half of `vals`), followed by J^T r and {cost, count}; `src[b]` = index among the travelling blocks of the one that
// holds block b's data (its own, or its mirror's for col < row).  One launch each way, a thread per double.
namespace dfh {
__global__ __launch_bounds__(256) void gn_pack_upper_kernel(const double *__restrict__ system, const int *__restrict__ row_of, const int *__restrict__ col,
                                                             const int *__restrict__ src, int n_blocks, int n_tail, double *__restrict__ packed,
                                                             int n_upper) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long nv = (long)n_blocks * 36;
    if (i < nv) {
        const int b = (int)(i / 36);
        if (col[b] >= row_of[b]) packed[(long)src[b] * 36 + (i - (long)b * 36)] = system[i];
    } else if (i < nv + n_tail) {
        packed[(long)n_upper * 36 + (i - nv)] = system[i];
    }
}
__global__ __launch_bounds__(256) void gn_unpack_upper_kernel(double *__restrict__ system, const int *__restrict__ row_of, const int *__restrict__ col,
                                                               const int *__restrict__ src, int n_blocks, int n_tail, const double *__restrict__ packed,
                                                               int n_upper) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long nv = (long)n_blocks * 36;
    if (i < nv) {
        const int b = (int)(i / 36), e = (int)(i - (long)b * 36);
        const bool upper = col[b] >= row_of[b];
        const int es = upper ? e : (e % 6) * 6 + e / 6;               // the mirror's entry (ib, ia)
        system[i] = packed[(long)src[b] * 36 + es];
    } else if (i < nv + n_tail) {
        system[i] = packed[(long)n_upper * 36 + (i - nv)];
    }
}
}  // namespace dfh

int dfh_gn_pack_upper(const double *system, const int *row_of, const int *col, const int *src, int n_blocks, int n_nodes, int n_upper,
                      double *packed, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(system && row_of && col && src && packed && n_blocks >= 0 && n_nodes >= 0 && n_upper >= 0, "dfh_gn_pack_upper: bad arguments");
    const long n = (long)n_blocks * 36 + 6L * n_nodes + 2;
    hipLaunchKernelGGL(gn_pack_upper_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, system, row_of, col, src,
                       n_blocks, 6 * n_nodes + 2, packed, n_upper);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_gn_unpack_upper(double *system, const int *row_of, const int *col, const int *src, int n_blocks, int n_nodes, int n_upper,
                        const double *packed, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(system && row_of && col && src && packed && n_blocks >= 0 && n_nodes >= 0 && n_upper >= 0, "dfh_gn_unpack_upper: bad arguments");
    const long n = (long)n_blocks * 36 + 6L * n_nodes + 2;
    hipLaunchKernelGGL(gn_unpack_upper_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, system, row_of, col, src,
                       n_blocks, 6 * n_nodes + 2, packed, n_upper);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

size_t dfh_gn_global_step_bytes(void) { return sizeof(double) * (42 * (size_t)dfh::kGlobalWgs + 2); }

int dfh_gn_global_step(const double *vals, int n_blocks, const double *rhs, int n_nodes, double lm_rel, double *node_dq, double *xi_out,
                       void *scratch, size_t scratch_bytes, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(vals && rhs && node_dq && scratch, "dfh_gn_global_step: null pointer");
    DFH_REQUIRE(n_blocks >= 1 && n_nodes >= 1 && lm_rel >= 0.0, "dfh_gn_global_step: bad sizes / damping");
    DFH_REQUIRE(scratch_bytes >= dfh_gn_global_step_bytes(), "dfh_gn_global_step: scratch too small (need %zu bytes, zeroed once)", dfh_gn_global_step_bytes());
    hipLaunchKernelGGL(gn_global_step_kernel, dim3(kGlobalWgs), dim3(256), 0, (hipStream_t)stream, vals, n_blocks, rhs, n_nodes, lm_rel, node_dq,
                       xi_out, static_cast<double *>(scratch));
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

size_t dfh_gn_global_sampled_bytes(int n_samples, int stride) {
    if (n_samples < 0 || stride < 1) return 0;
    return sizeof(double) * ((size_t)dfh::kGlobalVals * dfh::kGlobalGrid + 32);                                // workgroup partials | the 29 sums
}

int dfh_gn_global_apply(const double *sums29, double lm_rel, int n_nodes, double *node_dq, double *xi_out, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(sums29 && node_dq && n_nodes >= 1 && lm_rel >= 0.0, "dfh_gn_global_apply: bad arguments");
    hipLaunchKernelGGL(gn_global_apply_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sums29, lm_rel, n_nodes, node_dq, xi_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

// The body of dfh_gn_global_sampled / dfh_gn_global_sampled_volume.  views / vol: the association's arguments (one of them),
// f64: the maps' / the volume's type.  The problem and the frame or term are checked by the caller.
static int gn_global_sampled_impl(const char *what, const dfh_gn_problem &q, const dfh::AssocArgs *views, const dfh::VolAssocArgs *vol, bool f64,
                                  int stride, double lm_rel, int n_steps, double *xi_out, double *sums_out, void *scratch, size_t scratch_bytes,
                                  void *stream, const dfh::GatedAssocArgs *gated = nullptr) {
    using namespace dfh;
    const int n_samples = q.n_samples, knn = q.knn, n_nodes = q.n_nodes;
    DFH_REQUIRE(scratch && lm_rel >= 0.0, "%s: bad arguments", what);
    DFH_REQUIRE(scratch_bytes >= dfh_gn_global_sampled_bytes(n_samples, stride), "%s: scratch too small", what);
    DFH_REQUIRE(!sums_out || n_steps == 1, "%s: sums_out (the caller reduces over ranks and applies) takes one step per call", what);
    if (gated && n_samples == 0) return DFH_OK;                      // (nothing to gate: the ungated call is the one that writes empty sums)
    BuildParams bp;
    for (int i = 0; i < 8; ++i) bp.lw.q[i] = q.lw_dq[i];
    bp.S = n_samples; bp.k = knn; bp.N = n_nodes; bp.huber = q.huber_delta;
    const long n_tiles = (n_samples + kTile - 1) / kTile;
    const long n_sub = (n_tiles + stride - 1) / stride;
    const int n_wg = (int)std::min<long>(n_sub, kGlobalGrid);
    double *tile_part = static_cast<double *>(scratch);
    double *sums = sums_out ? sums_out : tile_part + (size_t)kGlobalVals * kGlobalGrid;
    hipStream_t st = (hipStream_t)stream;
    for (int g = 0; g < n_steps; ++g) {
        if (n_wg > 0) {
#define DFH_GLOBAL_ROWS_T(KK, T)                                                                                                   \
    if (vol)                                                                                                                       \
        hipLaunchKernelGGL((gn_global_rows_kernel<KK, T, true>), dim3((unsigned)n_wg), dim3(kTile), 0, st, q.sample_pos, q.sample_nrm,  \
                           q.nbr, q.weights, (const double *)q.node_dq, bp, stride, n_sub, tile_part, *vol);                         \
    else if (gated)                                                                                                                \
        hipLaunchKernelGGL((gn_global_rows_kernel<KK, T, false, true>), dim3((unsigned)n_wg), dim3(kTile), 0, st, q.sample_pos, q.sample_nrm, \
                           q.nbr, q.weights, (const double *)q.node_dq, bp, stride, n_sub, tile_part, *gated);                       \
    else                                                                                                                           \
        hipLaunchKernelGGL((gn_global_rows_kernel<KK, T>), dim3((unsigned)n_wg), dim3(kTile), 0, st, q.sample_pos, q.sample_nrm,        \
                           q.nbr, q.weights, (const double *)q.node_dq, bp, stride, n_sub, tile_part, *views)
#define DFH_GLOBAL_ROWS(KK)                                                                                                        \
    case KK:                                                                                                                       \
        if (f64) { DFH_GLOBAL_ROWS_T(KK, double); } else { DFH_GLOBAL_ROWS_T(KK, float); }                                         \
        break
            switch (knn) {
                DFH_GLOBAL_ROWS(1); DFH_GLOBAL_ROWS(2); DFH_GLOBAL_ROWS(3); DFH_GLOBAL_ROWS(4);
                DFH_GLOBAL_ROWS(5); DFH_GLOBAL_ROWS(6); DFH_GLOBAL_ROWS(7); DFH_GLOBAL_ROWS(8);
            }
#undef DFH_GLOBAL_ROWS
#undef DFH_GLOBAL_ROWS_T
        }
        if (sums_out) hipLaunchKernelGGL(gn_global_finish_kernel<false>, dim3(1), dim3(1024), 0, st, (const double *)tile_part, n_wg, sums, lm_rel, n_nodes, q.node_dq, xi_out);
        else hipLaunchKernelGGL(gn_global_finish_kernel<true>, dim3(1), dim3(1024), 0, st, (const double *)tile_part, n_wg, sums, lm_rel, n_nodes, q.node_dq, xi_out);
    }
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_gn_global_sampled(const dfh_gn_problem *problem, const dfh_gn_frame *frame, int stride, double lm_rel, int n_steps,
                          double *xi_out, double *sums_out, void *scratch, size_t scratch_bytes, void *stream) {
    using namespace dfh;
    const char *what = "dfh_gn_global_sampled";
    DFH_REQUIRE(n_steps >= 0 && n_steps <= 100 && stride >= 1, "%s: %d steps, stride %d", what, n_steps, stride);
    if (n_steps == 0) return DFH_OK;
    int rc = check_problem(what, problem, false);
    if (rc == DFH_OK) rc = check_frame(what, frame, false);
    if (rc != DFH_OK) return rc;
    const AssocArgs aa = assoc_args(*problem, *frame, false);
    return gn_global_sampled_impl(what, *problem, &aa, nullptr, frame->depth_dtype == DFH_F64, stride, lm_rel, n_steps, xi_out, sums_out,
                                  scratch, scratch_bytes, stream);
}

int dfh_gn_global_sampled_gated(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_normal_gate *gate, int stride,
                                double lm_rel, int n_steps, double *xi_out, double *sums_out, void *scratch, size_t scratch_bytes, void *stream) {
    using namespace dfh;
    const char *what = "dfh_gn_global_sampled_gated";
    DFH_REQUIRE(n_steps >= 0 && n_steps <= 100 && stride >= 1, "%s: %d steps, stride %d", what, n_steps, stride);
    if (n_steps == 0) return DFH_OK;
    int rc = check_problem(what, problem, false);
    if (rc == DFH_OK) rc = check_frame(what, frame, false);
    if (rc == DFH_OK) rc = check_gate(what, gate);
    if (rc != DFH_OK) return rc;
    const GatedAssocArgs ga = gated_assoc_args(*problem, *frame, *gate, false);
    return gn_global_sampled_impl(what, *problem, nullptr, nullptr, frame->depth_dtype == DFH_F64, stride, lm_rel, n_steps, xi_out, sums_out,
                                  scratch, scratch_bytes, stream, &ga);
}

int dfh_gn_global_sampled_volume(const dfh_gn_problem *problem, const dfh_gn_volume_term *term, int stride, double lm_rel, int n_steps,
                                 double *xi_out, double *sums_out, void *scratch, size_t scratch_bytes, void *stream) {
    using namespace dfh;
    const char *what = "dfh_gn_global_sampled_volume";
    DFH_REQUIRE(n_steps >= 0 && n_steps <= 100 && stride >= 1, "%s: %d steps, stride %d", what, n_steps, stride);
    if (n_steps == 0) return DFH_OK;
    int rc = check_problem(what, problem, false);
    if (rc == DFH_OK) rc = check_volume_term(what, term, false);
    if (rc != DFH_OK) return rc;
    const VolAssocArgs va = vol_assoc_args(*problem, *term);
    return gn_global_sampled_impl(what, *problem, nullptr, &va, term->live.dtype == DFH_F64, stride, lm_rel, n_steps, xi_out, sums_out,
                                  scratch, scratch_bytes, stream);
}

int dfh_relax_twists(double *node_dq, int n_nodes, double factor, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(n_nodes >= 0 && factor >= 0.0 && factor <= 1.0, "dfh_relax_twists: %d nodes, factor %g (0..1)", n_nodes, factor);
    if (n_nodes == 0 || factor == 1.0) return DFH_OK;
    DFH_REQUIRE(node_dq, "dfh_relax_twists: null pointer");
    hipLaunchKernelGGL(relax_twist_kernel, dim3((n_nodes + 255) / 256), dim3(256), 0, (hipStream_t)stream, node_dq, n_nodes, factor);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

}  // extern "C"
