// What the sparse terms of the warp-field solve share (K16 dfh_landmarks.hip, K18 dfh_photometric.hip; only those two include it).
//
// The scheme is the planned data term's.  A term's items arrive sorted by node tuple in tiles of kTile, the plan (dfh_plan.hip)
// gives every (tile, tuple) run a scratch row, and one workgroup per tile
//   1. gates its items and compacts the active ones in order (ballot + per-wave counts);
//   2. leaves at once when none is active: live flags 0, a {0, 0} cost pair;
//   3. adds the tile's objective in a fixed order into tile_cost;
//   4. finds the runs of equal scratch row in the compacted list, stores every run's row count and the tile's live flags;
//   5. stages rows [J | r] in LDS and STORES the Gram matrix of every run -- one wave per run, rows in ascending order, on the fp64
//      matrix cores -- to the run's scratch row.
// gn_gather_kernel then adds the live rows into the blocks with accumulate = true.  No floating-point atomics, a fixed order of
// every sum: the same bits every run.  A term brings its gate, its row (point_row with its own gradient vector) and what it keeps
// at a compacted position; the rest is here, once.
//
// gn_build_data_kernel (dfh_solve.hip) keeps its own copy of the scheme: it is benched, its register allocation has been tuned
// over several rounds, and lifting code out of a kernel has changed a sibling's allocation before (the note at the top of
// dfh_integrate_warped.hip).
#pragma once
#include "dfh_gn_rows.h"

#include <type_traits>

namespace dfh {

// Jacobian row of the point constraint g . x' with the vector g held constant, scaled by sc: data_row_from's gradient with n' = g
// and without the normal-rotation term.  g = e_a is one axis of a landmark, g = dI/dx' the photometric row.  k is the kernel's K
// as a function argument on purpose: as a template parameter it cost gn_photo_rows_kernel<1> 10 VGPRs and a wave per SIMD.
__device__ __forceinline__ void point_row(const double *__restrict__ node_dq, const int *idx, const double *w, int k, const double *lwq,
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

// Objective and row scale of an active item with squared residual norm q and weight s2: Huber on sqrt(q) when huber > 0.
__device__ __forceinline__ void robust_scale(double q, double s2, double huber, double &obj, double &sc) {
    if (huber > 0.0 && q > huber * huber) {
        const double n = sqrt(q);
        obj = s2 * huber * (n - 0.5 * huber);
        sc = sqrt(s2) * sqrt(huber / n);
    } else {
        obj = 0.5 * s2 * q;
        sc = sqrt(s2);
    }
}

// A tile's bookkeeping in LDS, for a workgroup of WAVES waves (at least kTile threads).
template <int WAVES>
struct TermTile {
    double obj[WAVES];
    int wave_cnt[WAVES];
    int run[kTile + 1];                 // run[0..n_runs]: the offsets in the compacted list where the scratch row changes
    int n_runs;
    int touched[kTile];
    unsigned short row[kTile];          // scratch row of every compacted item, relative to the tile's first
};

// Steps 1 and 2 for the tile of tile_n items from item blockIdx.x * kTile: `pos` is where this thread's active item goes in the
// compacted list of n_valid, [row_first, row_first + rows_tile) are the tile's scratch rows.  false: no item is active, the tile's
// live flags and cost pair are written, the workgroup returns.  One barrier.
template <int WAVES>
__device__ __forceinline__ bool term_tile_compact(TermTile<WAVES> &t, bool act, const int *__restrict__ run_id, int tile_n,
                                                  double *__restrict__ tile_cost, int n_tiles, int &pos, int &n_valid, int &row_first,
                                                  int &rows_tile) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned long long bal = __ballot(act);
    if (lane == 0) t.wave_cnt[wv] = __popcll(bal);
    __syncthreads();
    pos = __popcll(bal & ((1ull << lane) - 1ull));
    for (int w_ = 0; w_ < wv; ++w_) pos += t.wave_cnt[w_];
    n_valid = 0;
#pragma unroll
    for (int w_ = 0; w_ < WAVES; ++w_) n_valid += t.wave_cnt[w_];
    double *live = tile_cost + 2 * (size_t)n_tiles;
    row_first = run_id[blockIdx.x * kTile];
    rows_tile = run_id[blockIdx.x * kTile + tile_n - 1] - row_first + 1;
    if (n_valid == 0) {                                              // no active item: the tile's rows are dead
        if (tid < rows_tile) live[row_first + tid] = 0.0;
        if (tid == 0) { tile_cost[2 * blockIdx.x] = 0.0; tile_cost[2 * blockIdx.x + 1] = 0.0; }
        return false;
    }
    return true;
}

// Steps 3 and 4, after every active thread has stored t.row[pos]: returns the number of runs.  Four barriers; what the caller
// stored at its compacted positions before the call is visible to the workgroup after it.
template <int K, int WAVES>
__device__ __forceinline__ int term_tile_runs(TermTile<WAVES> &t, double obj, int n_valid, int row_first, int rows_tile,
                                              double *__restrict__ partial, double *__restrict__ tile_cost, int n_tiles) {
    constexpr int NJ = 6 * K, ST_ = gn_row_stride(K), NUP = gn_row_gram(K);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // the tile's objective, added in a fixed order; its count stays 0: cost_count[1] counts the data term's samples
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) obj += __shfl_xor(obj, o, 64);
    if (lane == 0) t.obj[wv] = obj;
    __syncthreads();
    if (tid == 0) {
        double o = t.obj[0];
#pragma unroll
        for (int w_ = 1; w_ < WAVES; ++w_) o += t.obj[w_];
        tile_cost[2 * blockIdx.x] = o;
        tile_cost[2 * blockIdx.x + 1] = 0.0;
    }
    const bool head = tid < n_valid && (tid == 0 || t.row[tid] != t.row[tid - 1]);
    const unsigned long long hb = __ballot(head);
    if (lane == 0) t.wave_cnt[wv] = __popcll(hb);         // (every thread passed the barrier after the first use)
    __syncthreads();
    int hp = __popcll(hb & ((1ull << lane) - 1ull));
    for (int w_ = 0; w_ < wv; ++w_) hp += t.wave_cnt[w_];
    if (head) t.run[hp] = tid;
    if (tid == 0) {
        int n = 0;
        for (int w_ = 0; w_ < WAVES; ++w_) n += t.wave_cnt[w_];
        t.run[n] = n_valid;
        t.n_runs = n;
    }
    if (tid < rows_tile) t.touched[tid] = 0;
    __syncthreads();
    const int n_runs = t.n_runs;
    if (tid < n_runs) {
        partial[(size_t)(row_first + t.row[t.run[tid]]) * ST_ + NUP + NJ + 1] = (double)(t.run[tid + 1] - t.run[tid]);
        t.touched[t.row[t.run[tid]]] = 1;
    }
    __syncthreads();
    double *live = tile_cost + 2 * (size_t)n_tiles;
    if (tid < rows_tile) live[row_first + tid] = t.touched[tid] ? 1.0 : 0.0;
    return n_runs;
}

// Step 5 for one run, by one wave: G = X^T X with X = rows [r0, r1) of sJ (6K + 1 doubles each, [J | r]) as 16 x 16 tiles of
// v_mfma_f64_16x16x4_f64, stored to the scratch row dst.  A run staged in several passes (CARRY) is carried through dst: with
// `carry` the accumulators -- the MFMA's C operand -- start from what the previous pass stored (an element belongs to one lane in
// every pass: a lane reads back its own store); `last`: the run is complete, its sum of r^2 is halved and the diagonal sub-blocks
// that straddle two 16 x 16 tiles are mirrored.
template <int K, bool CARRY>
__device__ __forceinline__ void gram_run(const double *sJ, int r0, int r1, bool carry, bool last, double *__restrict__ dst, int lane) {
    constexpr int NJ = 6 * K, LD = NJ + 1, NC = NJ + 1, NUP = gn_row_gram(K);
    constexpr int NT = (NC + 15) / 16;
    typedef double d4 __attribute__((ext_vector_type(4)));
    const int li = lane & 15, lk = lane >> 4;
    // where accumulator element (pa, pb) lives in the scratch row (-1: nowhere -- padding, or the lower half that is not kept)
    auto slot = [](int pa, int pb) -> int {
        if (pa < NJ && pb < NJ) {
            const int sa = pa / 6, sb = pb / 6;
            return sa <= sb ? 36 * gn_sub(K, sa, sb) + 6 * (pa - 6 * sa) + (pb - 6 * sb) : -1;
        }
        if (pa < NJ && pb == NJ) return NUP + pa;                    // J^T r
        if (pa == NJ && pb == NJ) return NUP + NJ;                   // sum of r^2 (halved when the run is complete)
        return -1;
    };
    d4 acc[NT * (NT + 1) / 2];
    {
        int q = 0;
#pragma unroll
        for (int bi = 0; bi < NT; ++bi)
#pragma unroll
            for (int bj = bi; bj < NT; ++bj, ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {                        // C/D: column = lane & 15, row = (lane >> 4) + 4 r
                    const int i = slot(16 * bi + lk + 4 * r, 16 * bj + li);
                    acc[q][r] = (CARRY && carry && i >= 0) ? dst[i] : 0.0;
                }
    }
    for (int t = r0; t < r1; t += 4) {
        double x[NT];                                                // A[i = li][k = lk] = B[k = lk][j = li] = X[t + lk][16 b + li]
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            const int c = 16 * b + li;
            const double *src = sJ + (t + lk) * LD + c;
            x[b] = (t + lk < r1 && c < NC) ? *src : 0.0;
        }
        int q = 0;
#pragma unroll
        for (int bi = 0; bi < NT; ++bi)
#pragma unroll
            for (int bj = bi; bj < NT; ++bj, ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[bi], x[bj], acc[q], 0, 0, 0);
    }
    int q = 0;
#pragma unroll
    for (int bi = 0; bi < NT; ++bi)
#pragma unroll
        for (int bj = bi; bj < NT; ++bj, ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pa = 16 * bi + lk + 4 * r, pb = 16 * bj + li;
                const int i = slot(pa, pb);
                const double v = acc[q][r];
                if (i >= 0) {
                    dst[i] = (last && pa == NJ) ? 0.5 * v : v;
                    // a diagonal sub-block that straddles two tiles: its lower entries lie in the tile that is not computed; the
                    // product is symmetric bit for bit
                    if (last && bi != bj && pb < NJ && pa / 6 == pb / 6)
                        dst[36 * gn_sub(K, pa / 6, pa / 6) + 6 * (pb - 6 * (pb / 6)) + (pa - 6 * (pa / 6))] = v;
                }
            }
}

// ------------------------------------------------------------------------------- host side
// The plan fields dfh_gn_landmarks and dfh_gn_photometric both carry.
struct TermPlan {
    const int *run_id;
    int n_rows;
    double *partial;                    // n_rows scratch rows | 2 doubles per tile | one live flag per row
    const int *blk_ptr, *blk_ent, *node_ptr, *node_ent;
};
template <typename T>
inline TermPlan term_plan(const T &t) {
    return TermPlan{t.run_id, t.n_rows, t.partial, t.blk_ptr, t.blk_ent, t.node_ptr, t.node_ent};
}

// A term of n items added to the problem's system: launch(K as a std::integral_constant, grid, tile_cost, n_tiles) queues the
// term's rows kernel for knn = K, then the gather adds the live rows into the blocks.
template <typename Launch>
inline int term_add(const dfh_gn_problem &q, const TermPlan &pl, int n, void *stream, Launch &&launch) {
    const int n_tiles = (n + kTile - 1) / kTile;
    double *tile_cost = pl.partial + (size_t)pl.n_rows * gn_row_stride(q.knn);
    const dim3 grid((unsigned)n_tiles);
#define DFH_TERM(KK) case KK: launch(std::integral_constant<int, KK>{}, grid, tile_cost, n_tiles); break
    switch (q.knn) {
        DFH_TERM(1); DFH_TERM(2); DFH_TERM(3); DFH_TERM(4); DFH_TERM(5); DFH_TERM(6); DFH_TERM(7); DFH_TERM(8);
    }
#undef DFH_TERM
    DFH_HIP_CHECK(hipGetLastError());
    const int *upper = (q.blk_upper && q.n_upper > 0 && !on(opt().gn_gather_full)) ? q.blk_upper : nullptr;
    return gn_gather_launch(q.knn, pl.partial, tile_cost + 2 * (size_t)n_tiles, pl.n_rows, pl.blk_ptr, pl.blk_ent, q.n_blocks, pl.node_ptr,
                            pl.node_ent, q.n_nodes, q.vals, q.rhs, q.cost_count, tile_cost, n_tiles, true, upper, q.n_upper, stream);
}

}  // namespace dfh
