// K14  exact nearest neighbour in descriptor space: dfh_nearest_descriptors (definition: include/dfusion_hip.h).
//
// Two paths, the same bits.
//   exact   nd_exact_kernel evaluates the definition for every pair: one query per thread with its channels in registers
//           (fp64), base rows staged through LDS and read as broadcasts, the running minimum per lane.
//   fast    the f32 score s~(q,l) = fl(|b_l|^2) - 2 a_q.b_l on the f32 matrix cores selects, per query, the few base rows that
//           can be the winner; those are re-evaluated with the definition.  Launch sequence, no host synchronisation:
//             nd_prep_base / nd_prep_query   padded operand images (below), |a_q|^2, B^2 = max |b_l|^2, the "unsafe" flags
//             nd_score_kernel<.., false>     smin[q] = min_l s~(q,l): running minimum per lane, an INTEGER atomic minimum on
//                                            the order-preserving image of the float per (wave, query)
//             nd_band_kernel                 thr[q] = smin[q] + 2 E_q rounded UP to float32 (E_q: "The guard band" below)
//             nd_score_kernel<.., true>      the same scores again (same operands, same k order, zero accumulator: the same
//                                            bits); every l with s~ <= thr[q] enters the query's candidate slots (an integer
//                                            atomic counter per query; kNdSlots slots)
//             nd_resolve_kernel              one thread per query: the definition on its candidates, lowest index on ties;
//                                            a query with more than kNdSlots candidates is flagged
//             nd_exact_kernel                the flagged queries
//           Nothing depends on the schedule: the minimum, the per-query candidate COUNT and the candidate SET are functions of
//           the inputs; the order of the slots is not, and the resolve step does not depend on it.
//
// Operand images (workspace).  K = 2 * steps floats per row, steps the smallest of {2, 4, 9, 17, 33} with 2 * steps >= dim + 1:
//   query row q:  (-2 a_q[0], ..., -2 a_q[dim-1], 1, 0, ...)       (the factor -2 is exact)
//   base row l:   (b_l[0], ..., b_l[dim-1], nb_l, 0, ...)          nb_l = float32(fp64 sum of squares of b_l)
// v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain, so with a zero accumulator
//   s~(q,l) = fl(fl(... fl(fl(-2 a_0 b_0) - 2 a_1 b_1) ... - 2 a_{dim-1} b_{dim-1}) + nb_l),
// and the padding steps fma(0, 0, acc) change nothing.  A base row with a NaN or an infinity never counts in the definition:
// its image is (0, ..., 0, +inf), its score +inf, above every finite threshold.  Rows past the end of either array likewise.
// The base is the A operand (rows of the 32 x 32 tile), the queries are B (columns): lane & 31 is the lane's query, its 16
// accumulator registers are 16 base rows, and the minimum over the base never leaves the lane until the tile walk ends.
//
// The guard band.  u = 2^-24, D = dim, real arithmetic unless "fl".  Write s(q,l) = |b_l|^2 - 2 a_q.b_l, so that the real squared
// distance is |a_q|^2 + s(q,l), and B = max |b_l| over the base rows that count.
//  (1) The score.  The chain rounds D + 1 times, each rounding relative u of a partial sum that is at most
//      (1 + u)^(D+1) (sum_c |2 a_c b_c| + nb_l); sum_c |2 a_c b_c| <= 2 |a_q| B (Cauchy-Schwarz).  nb_l is within
//      (u + (D + 1) 2^-53)(1 + 2^-50) |b_l|^2 of |b_l|^2.  A rounding that lands in the float32 subnormals adds at most 2^-150.  So
//        |s~ - s| <= E1 := 1.01 (D + 3) u (2 |a_q| B + B^2) + 2^-140          ((D + 1) u <= 65 * 2^-24 < 4e-6: 1.01 covers
//      the (1 + u)^(D+1) factors and the fp64 roundings of |a_q|, B themselves),
//      PROVIDED no intermediate overflows: the kernels require |a_q| < 2^62, B^2 < 2^124 -- "safe" below -- whence every
//      partial sum stays below 2^127.
//  (2) The definition.  t_c = fl(a_c - b_c) is within 2^-53 relative, fl(t_c t_c) another 2^-53 (no underflow: a non-zero
//      difference of two float32 is at least 2^-149, its square 2^-298; no overflow: |t_c| < 2^129), and the D - 1 additions of
//      non-negative terms 2^-53 each:  |d2 - (|a_q|^2 + s)| <= g (|a_q| + B)^2,  g := 1.01 (D + 2) 2^-53.
//  (3) Let w be the definition's winner of query q and m the row with the smallest score.  d2(w) <= d2(m) gives, by (2),
//      s(w) <= s(m) + 2 g (|a_q| + B)^2, and by (1) twice  s~(w) <= s~(m) + 2 E1 + 2 g (|a_q| + B)^2 = smin + 2 E_q with
//        E_q := E1 + g (|a_q| + B)^2.
//      Every row that ties with w in d2 satisfies the same inequality, so the lowest tied index is among the candidates too.
//      thr[q] is smin + 2 E_q evaluated in fp64 (the 1.01 above leaves room for those roundings) and rounded UP to float32:
//      the candidates are a superset of the band, which only ever costs re-evaluations.
// Not safe: a query with a NaN / infinity or |a_q| >= 2^62 is flagged for the exact kernel; a finite base row with
// |b_l|^2 >= 2^124 sets one flag that sends EVERY query there (such a row counts in the definition and has no finite score).
// A query whose smin is +inf (no base row counts) is flagged as well; the exact kernel gives it -1 / +inf.
#include <cmath>
#include <cstdint>

#include "dfh_common.h"

namespace dfh {

typedef float nd_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kNdSlots = 32;          // candidate slots per query; more candidates than that: the exact kernel
constexpr int kNdTileQ = 128;         // queries per workgroup of the score kernel (4 waves x 32)
constexpr int kNdTileB = 128;         // base rows per LDS chunk (4 sub-tiles of 32)
constexpr int kNdExactQ = 256;        // queries per workgroup of the exact kernel (one per thread)
constexpr int kNdExactFloats = 4096;  // LDS floats of one staged base chunk of the exact kernel
constexpr unsigned kNdEncNone = 0xffffffffu;

__host__ __device__ inline int nd_steps(int dim) {
    const int need = dim + 1;
    return need <= 4 ? 2 : need <= 8 ? 4 : need <= 18 ? 9 : need <= 34 ? 17 : 33;
}
__host__ __device__ inline long nd_pad(long n, long m) { return (n + m - 1) / m * m; }

struct NdHeader {                     // cleared by one memset
    unsigned long long b2max_bits;    // max over the counting base rows of fp64 |b_l|^2 (bits; non-negative doubles order as integers)
    unsigned long long pairs;         // stats_out[0]
    unsigned long long handed;        // stats_out[1]
    unsigned int base_unsafe;         // a finite base row without a finite score
    unsigned int pad;
};

struct NdLayout {
    size_t hdr, smin, count, flag, thr, qn2, cand, qimg, bimg, end;
};

static NdLayout nd_layout(long nq, long nb, int dim) {
    NdLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 15) / 16 * 16; return at; };
    const size_t K = 2 * (size_t)nd_steps(dim);
    const size_t nqp = (size_t)nd_pad(nq, kNdTileQ), nbp = (size_t)nd_pad(nb, kNdTileB);
    L.hdr = take(sizeof(NdHeader));
    L.smin = take(4 * nqp);           // hdr, smin, count, flag are adjacent: one memset pattern each
    L.count = take(4 * nqp);
    L.flag = take(4 * nqp);
    L.thr = take(4 * nqp);
    L.qn2 = take(8 * nqp);
    L.cand = take(4 * (size_t)kNdSlots * nqp);
    L.qimg = take(4 * K * nqp);
    L.bimg = take(4 * K * nbp);
    L.end = o;
    return L;
}

__device__ __forceinline__ unsigned nd_enc(float f) {               // order-preserving float -> unsigned
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float nd_dec(unsigned e) {
    return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

// ---- operand images --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nd_prep_base(const float *__restrict__ base, long nb, long nb_pad, int dim, int K,
                                                    float *__restrict__ bimg, NdHeader *__restrict__ hdr) {
    const long l = (long)blockIdx.x * 256 + threadIdx.x;
    if (l >= nb_pad) return;
    float *row = bimg + (size_t)l * K;
    bool counts = l < nb;
    double n2 = 0.0;
    if (counts) {
        const float *b = base + (size_t)l * dim;
        for (int c = 0; c < dim; ++c) {
            const double v = (double)b[c];
            counts = counts && fabs(v) <= 3.5e38;                     // (false for a NaN, true for every finite float32)
            n2 += v * v;
        }
    }
    if (counts && !(n2 < 0x1p124)) {                                 // counts in the definition, has no finite score
        hdr->base_unsafe = 1u;                                       // (every writer stores the same word)
        counts = false;
    }
    if (counts) {
        const float *b = base + (size_t)l * dim;
        for (int c = 0; c < dim; ++c) row[c] = b[c];
        row[dim] = (float)n2;
        for (int c = dim + 1; c < K; ++c) row[c] = 0.0f;
        atomicMax(&hdr->b2max_bits, (unsigned long long)__double_as_longlong(n2));
    } else {
        for (int c = 0; c < K; ++c) row[c] = 0.0f;
        row[dim] = __builtin_huge_valf();
    }
}

__global__ __launch_bounds__(256) void nd_prep_query(const float *__restrict__ query, long nq, long nq_pad, int dim, int K,
                                                     float *__restrict__ qimg, double *__restrict__ qn2,
                                                     unsigned *__restrict__ flag) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq_pad) return;
    float *row = qimg + (size_t)q * K;
    bool safe = q < nq;
    double n2 = 0.0;
    if (safe) {
        const float *a = query + (size_t)q * dim;
        for (int c = 0; c < dim; ++c) {
            const double v = (double)a[c];
            safe = safe && fabs(v) <= 3.5e38;
            n2 += v * v;
        }
        safe = safe && n2 < 0x1p124;                                  // |a_q| < 2^62
        if (!safe) flag[q] = 1u;
    }
    if (safe) {
        const float *a = query + (size_t)q * dim;
        for (int c = 0; c < dim; ++c) row[c] = -2.0f * a[c];
        row[dim] = 1.0f;
        for (int c = dim + 1; c < K; ++c) row[c] = 0.0f;
    } else {
        for (int c = 0; c < K; ++c) row[c] = 0.0f;
    }
    qn2[q] = n2;
}

// ---- the scores on the matrix cores ------------------------------------------------------------------------------------------
// grid (query tiles, base splits); a workgroup walks the base chunks y, y + gridDim.y, ...; wave w owns queries q0 + 32 w ..
template <int STEPS, bool EMIT>
__global__ __launch_bounds__(256) void nd_score_kernel(const float *__restrict__ qimg, const float *__restrict__ bimg, long nq,
                                                       long nb, long nb_pad, const NdHeader *__restrict__ hdr,
                                                       unsigned *__restrict__ smin, const float *__restrict__ thr,
                                                       unsigned *__restrict__ count, int *__restrict__ cand) {
    constexpr int K = 2 * STEPS;
    constexpr int S = (STEPS & 1) ? K : K + 2;                       // LDS row stride: 2 x odd words, so that the 32 rows a
    __shared__ float sB[kNdTileB * S];                               // half-wave reads fall into 32 different even banks
    if (hdr->base_unsafe) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int col = lane & 31, half = lane >> 5;
    const long q = (long)blockIdx.x * kNdTileQ + wv * 32 + col;      // (< nq_pad: the image has the row)
    float a[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) a[s] = qimg[(size_t)q * K + 2 * s + half];
    float best = __builtin_huge_valf();
    float limit = -__builtin_huge_valf();
    if (EMIT && q < nq) limit = thr[q];

    const long n_chunks = nb_pad / kNdTileB;
    for (long ch = blockIdx.y; ch < n_chunks; ch += gridDim.y) {
        __syncthreads();
        const float *src = bimg + (size_t)ch * kNdTileB * K;
        for (int i = threadIdx.x; i < kNdTileB * K; i += 256) sB[(i / K) * S + (i % K)] = src[i];
        __syncthreads();
#pragma unroll 1
        for (int sub = 0; sub < kNdTileB / 32; ++sub) {
            nd_f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            const float *rowp = sB + (sub * 32 + col) * S + half;
#pragma unroll
            for (int s = 0; s < STEPS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(rowp[2 * s], a[s], acc, 0, 0, 0);
            if (!EMIT) {
#pragma unroll
                for (int r = 0; r < 16; ++r) best = fminf(best, acc[r]);
            } else {
                const long l0 = ch * kNdTileB + sub * 32 + 4 * half;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (acc[r] <= limit) {                           // (rare: about one pair per query)
                        const long l = l0 + (r & 3) + 8 * (r >> 2);
                        if (l < nb) {
                            const unsigned slot = atomicAdd(count + q, 1u);
                            if (slot < (unsigned)kNdSlots) cand[(size_t)q * kNdSlots + slot] = (int)l;
                        }
                    }
                }
            }
        }
    }
    if (!EMIT) {
        best = fminf(best, __shfl_xor(best, 32, 64));
        if (half == 0 && q < nq) atomicMin(smin + q, nd_enc(best));
    }
}

// ---- thr[q] = smin[q] + 2 E_q, rounded up to float32 -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nd_band_kernel(long nq, int dim, const NdHeader *__restrict__ hdr,
                                                      const unsigned *__restrict__ smin, const double *__restrict__ qn2,
                                                      unsigned *__restrict__ flag, float *__restrict__ thr) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq || hdr->base_unsafe) return;
    if (flag[q]) { thr[q] = -__builtin_huge_valf(); return; }
    const unsigned e = smin[q];
    const float sm = nd_dec(e);
    if (e == kNdEncNone || !(fabsf(sm) <= 3.0e38f)) {                // no base row counts (or nothing arrived): the exact kernel
        flag[q] = 1u;
        thr[q] = -__builtin_huge_valf();
        return;
    }
    const double B2 = __longlong_as_double((long long)hdr->b2max_bits);
    const double B = sqrt(B2), A = sqrt(qn2[q]);
    const double e1 = 1.01 * (double)(dim + 3) * 0x1p-24 * (2.0 * A * B + B2) + 0x1p-140;
    const double g = 1.01 * (double)(dim + 2) * 0x1p-53;
    const double eq = e1 + g * ((A + B) * (A + B));
    const double t = (double)sm + 2.0 * eq;
    float tf = (float)t;
    if ((double)tf < t) tf = nextafterf(tf, __builtin_huge_valf());
    thr[q] = tf;
}

// ---- the definition, one pair ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double nd_d2(const float *__restrict__ a, const float *__restrict__ b, int dim) {
    double d2 = 0.0;
    for (int c = 0; c < dim; ++c) {
        const double t = (double)a[c] - (double)b[c];
        const double p = t * t;
        d2 = c == 0 ? p : d2 + p;
    }
    return d2;
}

__global__ __launch_bounds__(256) void nd_resolve_kernel(const float *__restrict__ query, long nq, const float *__restrict__ base,
                                                         int dim, NdHeader *__restrict__ hdr, const unsigned *__restrict__ count,
                                                         const int *__restrict__ cand, unsigned *__restrict__ flag,
                                                         int *__restrict__ idx_out, double *__restrict__ d2_out) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long pairs = 0, handed = 0;
    if (q < nq) {
        const unsigned n = count[q];
        if (hdr->base_unsafe || flag[q] || n == 0u || n > (unsigned)kNdSlots) {
            flag[q] = 1u;
            handed = 1;
        } else {
            const float *a = query + (size_t)q * dim;
            double best = __builtin_huge_val();
            int arg = -1;
            for (unsigned i = 0; i < n; ++i) {
                const int l = cand[(size_t)q * kNdSlots + i];
                const double d2 = nd_d2(a, base + (size_t)l * dim, dim);
                if (d2 < best || (d2 == best && l < arg)) { best = d2; arg = l; }
            }
            idx_out[q] = arg;
            if (d2_out) d2_out[q] = best;
            pairs = n;
        }
    }
    // integer sums: the order of the additions does not matter
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        pairs += __shfl_xor(pairs, o, 64);
        handed += __shfl_xor(handed, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (pairs) atomicAdd(&hdr->pairs, pairs);
        if (handed) atomicAdd(&hdr->handed, handed);
    }
}

__global__ void nd_stats_kernel(const NdHeader *__restrict__ hdr, long *__restrict__ stats) {
    if (threadIdx.x == 0) {
        stats[0] = (long)hdr->pairs;
        stats[1] = (long)hdr->handed;
    }
}

__global__ void nd_stats_exact_kernel(long nq, long *__restrict__ stats) {
    if (threadIdx.x == 0) {
        stats[0] = 0;
        stats[1] = nq;
    }
}

// ---- the exact kernel: every pair, or every pair of the flagged queries (flag != NULL) -----------------------------------------
template <int DB>
__global__ __launch_bounds__(kNdExactQ) void nd_exact_kernel(const float *__restrict__ query, long nq, const float *__restrict__ base,
                                                              long nb, int dim, const unsigned *__restrict__ flag,
                                                              int *__restrict__ idx_out, double *__restrict__ d2_out) {
    __shared__ float sB[kNdExactFloats];
    const long q = (long)blockIdx.x * kNdExactQ + threadIdx.x;
    const bool mine = q < nq && (!flag || flag[q] != 0u);
    if (!__syncthreads_or(mine)) return;                             // nothing flagged in this workgroup
    double a[DB];
#pragma unroll
    for (int c = 0; c < DB; ++c) a[c] = (mine && c < dim) ? (double)query[(size_t)q * dim + c] : 0.0;
    const int rows = kNdExactFloats / dim;                           // dim <= 64: at least 64 rows
    double best = __builtin_huge_val();
    int arg = -1;
    for (long l0 = 0; l0 < nb; l0 += rows) {
        const int nr = (int)((nb - l0) < (long)rows ? (nb - l0) : (long)rows);
        __syncthreads();
        const float *src = base + (size_t)l0 * dim;
        for (int i = threadIdx.x; i < nr * dim; i += kNdExactQ) sB[i] = src[i];
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            const float *b = sB + r * dim;                           // (the same address in every lane: a broadcast)
            double d2 = 0.0;
#pragma unroll
            for (int c = 0; c < DB; ++c) {
                if (c < dim) {
                    const double t = a[c] - (double)b[c];
                    const double p = t * t;
                    d2 = c == 0 ? p : d2 + p;
                }
            }
            if (d2 < best) { best = d2; arg = (int)(l0 + r); }       // (false for a NaN and for +inf; ascending l: lowest index on ties)
        }
    }
    if (mine) {
        idx_out[q] = arg;
        if (d2_out) d2_out[q] = best;
    }
}

static void nd_launch_exact(hipStream_t s, const float *query, long nq, const float *base, long nb, int dim, const unsigned *flag,
                            int *idx_out, double *d2_out) {
    const dim3 grid((unsigned)((nq + kNdExactQ - 1) / kNdExactQ)), block(kNdExactQ);
    if (dim <= 4) hipLaunchKernelGGL(nd_exact_kernel<4>, grid, block, 0, s, query, nq, base, nb, dim, flag, idx_out, d2_out);
    else if (dim <= 16) hipLaunchKernelGGL(nd_exact_kernel<16>, grid, block, 0, s, query, nq, base, nb, dim, flag, idx_out, d2_out);
    else hipLaunchKernelGGL(nd_exact_kernel<64>, grid, block, 0, s, query, nq, base, nb, dim, flag, idx_out, d2_out);
}

template <bool EMIT>
static void nd_launch_score(hipStream_t s, int steps, dim3 grid, const float *qimg, const float *bimg, long nq, long nb, long nb_pad,
                            const NdHeader *hdr, unsigned *smin, const float *thr, unsigned *count, int *cand) {
    const dim3 block(256);
#define DFH_ND_CASE(N)                                                                                                          \
    case N:                                                                                                                     \
        hipLaunchKernelGGL((nd_score_kernel<N, EMIT>), grid, block, 0, s, qimg, bimg, nq, nb, nb_pad, hdr, smin, thr, count, cand); \
        break;
    switch (steps) {
        DFH_ND_CASE(2) DFH_ND_CASE(4) DFH_ND_CASE(9) DFH_ND_CASE(17) DFH_ND_CASE(33)
    }
#undef DFH_ND_CASE
}

static const char *nd_check_sizes(long nq, long nb, int dim) {
    if (dim < 1 || dim > 64) return "dim outside 1..64";
    if (nb < 1 || nb >= (1L << 31)) return "n_base outside [1, 2^31)";
    if (nq < 0 || nq >= (1L << 31)) return "n_query outside [0, 2^31)";
    return nullptr;
}

// The library's own choice (nd_path unset).  Measured (profiles/r14_descriptors.txt): the fast path beat the exact kernel at every
// size timed, from 64 x 64 pairs (48 against 56 us, twins equal to the microsecond) to the 512^3 scene's 77 k x 787 k (12x).
// Below the smallest size measured the exact kernel's single launch stays.
static int nd_choose(long nq, long nb, int dim) {
    (void)dim;
    const long v = opt().nd_path;
    if (v == 1 || v == 2) return (int)v;
    return (double)nq * (double)nb >= 4096.0 ? 2 : 1;
}

}  // namespace dfh

// =================================================================================== C ABI
extern "C" {

size_t dfh_nearest_descriptors_workspace_bytes(long n_query, long n_base, int dim) {
    if (dfh::nd_check_sizes(n_query, n_base, dim) || n_query == 0) return 0;
    return dfh::nd_layout(n_query, n_base, dim).end;
}

int dfh_nearest_descriptors_tile(int tile[4]) {
    using namespace dfh;
    DFH_REQUIRE(tile, "dfh_nearest_descriptors_tile: null output");
    tile[0] = kNdTileQ;
    tile[1] = kNdTileB;
    tile[2] = kNdExactQ;
    tile[3] = kNdSlots;
    return DFH_OK;
}

int dfh_nearest_descriptors_path(long n_query, long n_base, int dim) {
    using namespace dfh;
    const char *bad = nd_check_sizes(n_query, n_base, dim);
    DFH_REQUIRE(!bad, "dfh_nearest_descriptors_path: %s (n_query=%ld, n_base=%ld, dim=%d)", bad, n_query, n_base, dim);
    return nd_choose(n_query, n_base, dim);
}

int dfh_nearest_descriptors(const float *query, long n_query, const float *base, long n_base, int dim, int *idx_out, double *d2_out,
                            long *stats_out, void *workspace, size_t workspace_bytes, void *stream) {
    using namespace dfh;
    const char *bad = nd_check_sizes(n_query, n_base, dim);
    DFH_REQUIRE(!bad, "dfh_nearest_descriptors: %s (n_query=%ld, n_base=%ld, dim=%d)", bad, n_query, n_base, dim);
    const long v = opt().nd_path;
    DFH_REQUIRE(v < 0 || v == 1 || v == 2, "dfh_nearest_descriptors: option nd_path=%ld is not 1 (exact) or 2 (fast)", v);
    if (n_query == 0) return DFH_OK;
    DFH_REQUIRE(query && base && idx_out, "dfh_nearest_descriptors: null pointer");
    const int path = nd_choose(n_query, n_base, dim);
    hipStream_t s = (hipStream_t)stream;
    if (path == 1) {
        nd_launch_exact(s, query, n_query, base, n_base, dim, nullptr, idx_out, d2_out);
        if (stats_out) hipLaunchKernelGGL(nd_stats_exact_kernel, dim3(1), dim3(64), 0, s, n_query, stats_out);
        DFH_HIP_CHECK(hipGetLastError());
        return DFH_OK;
    }
    const NdLayout L = nd_layout(n_query, n_base, dim);
    DFH_REQUIRE(workspace, "dfh_nearest_descriptors: null workspace");
    DFH_REQUIRE(workspace_bytes >= L.end, "dfh_nearest_descriptors: workspace too small (%zu < %zu bytes)", workspace_bytes, L.end);
    DFH_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "dfh_nearest_descriptors: workspace must be 16-byte aligned");
    char *ws = static_cast<char *>(workspace);
    NdHeader *hdr = reinterpret_cast<NdHeader *>(ws + L.hdr);
    unsigned *smin = reinterpret_cast<unsigned *>(ws + L.smin);
    unsigned *count = reinterpret_cast<unsigned *>(ws + L.count);
    unsigned *flag = reinterpret_cast<unsigned *>(ws + L.flag);
    float *thr = reinterpret_cast<float *>(ws + L.thr);
    double *qn2 = reinterpret_cast<double *>(ws + L.qn2);
    int *cand = reinterpret_cast<int *>(ws + L.cand);
    float *qimg = reinterpret_cast<float *>(ws + L.qimg);
    float *bimg = reinterpret_cast<float *>(ws + L.bimg);
    const int steps = nd_steps(dim), K = 2 * steps;
    const long nqp = nd_pad(n_query, kNdTileQ), nbp = nd_pad(n_base, kNdTileB);

    DFH_HIP_CHECK(hipMemsetAsync(hdr, 0, sizeof(NdHeader), s));
    DFH_HIP_CHECK(hipMemsetAsync(smin, 0xff, L.count - L.smin, s));
    DFH_HIP_CHECK(hipMemsetAsync(count, 0, L.thr - L.count, s));                     // count and flag
    hipLaunchKernelGGL(nd_prep_base, dim3((unsigned)((nbp + 255) / 256)), dim3(256), 0, s, base, n_base, nbp, dim, K, bimg, hdr);
    hipLaunchKernelGGL(nd_prep_query, dim3((unsigned)((nqp + 255) / 256)), dim3(256), 0, s, query, n_query, nqp, dim, K, qimg, qn2, flag);
    // base splits: enough workgroups to fill the device when there are few query tiles (the result does not depend on it)
    const long q_tiles = nqp / kNdTileQ, chunks = nbp / kNdTileB;
    long splits = (2048 + q_tiles - 1) / q_tiles;
    if (splits > chunks) splits = chunks;
    if (splits > 65535) splits = 65535;
    if (splits < 1) splits = 1;
    const dim3 grid((unsigned)q_tiles, (unsigned)splits);
    const unsigned qblocks = (unsigned)((n_query + 255) / 256);
    nd_launch_score<false>(s, steps, grid, qimg, bimg, n_query, n_base, nbp, hdr, smin, thr, count, cand);
    hipLaunchKernelGGL(nd_band_kernel, dim3(qblocks), dim3(256), 0, s, n_query, dim, hdr, smin, qn2, flag, thr);
    nd_launch_score<true>(s, steps, grid, qimg, bimg, n_query, n_base, nbp, hdr, smin, thr, count, cand);
    hipLaunchKernelGGL(nd_resolve_kernel, dim3(qblocks), dim3(256), 0, s, query, n_query, base, dim, hdr, count, cand, flag, idx_out, d2_out);
    nd_launch_exact(s, query, n_query, base, n_base, dim, flag, idx_out, d2_out);
    if (stats_out) hipLaunchKernelGGL(nd_stats_kernel, dim3(1), dim3(64), 0, s, hdr, stats_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

}  // extern "C"
