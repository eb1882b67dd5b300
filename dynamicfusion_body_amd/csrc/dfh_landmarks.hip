// K16: the landmark term of the warp-field solve -- point-to-point rows for feature correspondences (include/dfusion_hip.h:
// dfh_gn_landmarks; restated in tests/landmark_np.py).
//
// A landmark is a canonical point with a live 3-D target: three rows sc (x' - c)_a, a = 0, 1, 2, where the data term has the one
// row n'.(x' - c).  The rows reuse everything the planned data term has: landmarks arrive sorted by node tuple in tiles of kTile,
// the plan (dfh_plan.hip) gives every (tile, tuple) run a scratch row, this kernel STORES each run's Gram matrix there (the fp64
// matrix cores, as gn_build_data_kernel does it) and gn_gather_kernel adds the rows into the blocks with accumulate = true.  No
// floating-point atomics, the same bits every run.
//
// A run's rows are 3 n x (6K + 1): three times the data term's LDS if staged whole (150 KB at K = 8).  The tile's active landmarks
// are therefore staged kTile / 3 at a time, each with its three axis rows side by side: pass c holds the rows of compacted
// landmarks [CH c, CH c + CH), CH = kTile / 3, one (landmark, axis) pair per thread -- the pair's thread warps the landmark again (the same
// functions on the same values as the gate's pass: the same bits) and differentiates its axis.  A run's accumulators take its rows
// in the fixed order landmark by landmark, axis 0, 1, 2.  A run that a pass boundary cuts (at most one per boundary) is carried
// through its scratch row: the next pass starts its accumulators -- the MFMA's C operand -- from what the previous one stored; the
// run belongs to one wave and an accumulator element to one lane in every pass, so the reload is a lane reading back its own store.
#include "dfh_gn_rows.h"

#include <cmath>

namespace dfh {

struct LandmarkParams {
    DQ lw;
    int n;
    double weight, huber, max_dist;
};

// Jacobian row of axis a of one landmark: data_row_from's gradient with n' = e_a and without the normal-rotation term.
__device__ __forceinline__ void landmark_axis_row(const double *__restrict__ node_dq, const int *idx, const double *w, int k, const double *lwq,
                                                  const double *bh, double nb, double pfx, double pfy, double pfz, int a, double sc,
                                                  double *Jrow) {
    const Q4 rl{lwq[0], lwq[1], lwq[2], lwq[3]};
    const Q4 rlc = qconj(rl);
    const Q4 U = qmul(qmul(rlc, qpure(a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0)), rl);
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

// What the term needs of one landmark: its nodes, the normalised blend, the float32-rounded point, d = x' - c, whether it is active,
// and then its objective and the scale of its three rows (dfusion_hip.h, steps 1-4).
struct LandmarkState {
    int idx[kKMaxS];
    double w[kKMaxS];
    double bh[8], nb, pf[3], d[3], sc, obj;
    bool act;
};
template <int K>
__device__ __forceinline__ void landmark_state(int s, const double *__restrict__ lpos, const int *__restrict__ nbr, const double *__restrict__ wts,
                                               const double *__restrict__ target, const unsigned char *__restrict__ valid,
                                               const double *__restrict__ conf, const double *__restrict__ node_dq, const LandmarkParams &p,
                                               LandmarkState &st) {
#pragma unroll
    for (int j = 0; j < kKMaxS; ++j) {
        st.idx[j] = j < K ? nbr[(size_t)s * K + j] : 0;
        st.w[j] = j < K ? wts[(size_t)s * K + j] : 0.0;
    }
    st.nb = blend_static(node_dq, st.idx, st.w, K, st.bh);
    st.pf[0] = round_f32(lpos[3 * (size_t)s]); st.pf[1] = round_f32(lpos[3 * (size_t)s + 1]); st.pf[2] = round_f32(lpos[3 * (size_t)s + 2]);
    const D3 x1 = dqb_warp_exact(st.bh, st.pf[0], st.pf[1], st.pf[2]);
    const D3 xp = dqb_warp_exact(p.lw.q, round_f32(x1.x), round_f32(x1.y), round_f32(x1.z));
    st.d[0] = xp.x - target[3 * (size_t)s]; st.d[1] = xp.y - target[3 * (size_t)s + 1]; st.d[2] = xp.z - target[3 * (size_t)s + 2];
    const double q = (st.d[0] * st.d[0] + st.d[1] * st.d[1]) + st.d[2] * st.d[2];
    const double s2 = p.weight * (conf ? conf[s] : 1.0);
    st.act = (valid ? valid[s] != 0 : true) && s2 > 0.0 && q < __builtin_huge_val() &&            // (a NaN fails)
             (p.max_dist <= 0.0 || q <= p.max_dist * p.max_dist);
    st.sc = 0.0; st.obj = 0.0;
    if (st.act) {
        if (p.huber > 0.0 && q > p.huber * p.huber) {              // vector Huber on |d|
            const double n = sqrt(q);
            st.obj = s2 * p.huber * (n - 0.5 * p.huber);
            st.sc = sqrt(s2) * sqrt(p.huber / n);
        } else {
            st.obj = 0.5 * s2 * q;
            st.sc = sqrt(s2);
        }
    }
}

// One kTile-landmark tile per workgroup; writes dfh_gn_problem.partial's layout: the tile's scratch rows, its {cost, 0} pair
// (tile_cost) and its rows' live flags (behind the n_tiles pairs).  The workgroup has twice the tile's threads: sparse landmarks
// share few node tuples, a tile holds tens of runs, and the Gram phase -- one wave per run, one run after the other -- sets the
// tile's duration; threads kTile.. only take part in it (19 k landmarks are 149 tiles: the extra waves' CUs were idle anyway).
constexpr int kLmThreads = 2 * kTile, kLmWaves = kLmThreads / 64;
template <int K>
__global__ __launch_bounds__(kLmThreads) void gn_landmark_rows_kernel(const double *__restrict__ lpos, const int *__restrict__ nbr,
                                                                const double *__restrict__ wts, const double *__restrict__ target,
                                                                const unsigned char *__restrict__ valid, const double *__restrict__ conf,
                                                                const double *__restrict__ node_dq, const LandmarkParams p,
                                                                const int *__restrict__ run_id, double *__restrict__ partial,
                                                                double *__restrict__ tile_cost, int n_tiles,
                                                                unsigned char *__restrict__ active_out) {
    constexpr int NJ = 6 * K;                   // Jacobian entries per row
    constexpr int LD = NJ + 1;                  // + residual
    constexpr int ST_ = gn_row_stride(K);
    constexpr int NUP = gn_row_gram(K);
    constexpr int CH = kTile / 3;               // landmarks per pass: 3 CH rows, one per thread
    __shared__ double sJ[3 * CH * LD];          // one pass' rows: compacted landmark c0 + i, axis a in row 3 i + a
    __shared__ int sWaveCnt[kLmWaves];
    __shared__ unsigned short sRow[kTile];      // scratch row of every compacted landmark, relative to the tile's first
    __shared__ unsigned short sSrc[kTile];      // ... and the thread (= landmark of the tile) it came from
    __shared__ double sObj[kLmWaves];
    __shared__ int sRun[kTile + 1];
    __shared__ int sNRuns;
    __shared__ int sTouched[kTile];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int s = blockIdx.x * kTile + tid;
    const int tile_n = min(kTile, p.n - blockIdx.x * kTile);
    bool act = false;
    double obj = 0.0;
    if (tid < tile_n) {
        LandmarkState st;
        landmark_state<K>(s, lpos, nbr, wts, target, valid, conf, node_dq, p, st);
        act = st.act;
        obj = st.obj;
        if (active_out) active_out[s] = act ? 1 : 0;
    }
    // the active landmarks, compacted in order (gn_build_data_kernel's scheme)
    const unsigned long long bal = __ballot(act);
    if (lane == 0) sWaveCnt[wv] = __popcll(bal);
    __syncthreads();
    int pos = __popcll(bal & ((1ull << lane) - 1ull));
    for (int w_ = 0; w_ < wv; ++w_) pos += sWaveCnt[w_];
    int n_valid = 0;
#pragma unroll
    for (int w_ = 0; w_ < kLmWaves; ++w_) n_valid += sWaveCnt[w_];
    double *live = tile_cost + 2 * (size_t)n_tiles;
    const int row_first = run_id[blockIdx.x * kTile];
    const int rows_tile = run_id[blockIdx.x * kTile + tile_n - 1] - row_first + 1;
    if (n_valid == 0) {                                              // no active landmark: the tile's rows are dead
        if (tid < rows_tile) live[row_first + tid] = 0.0;
        if (tid == 0) { tile_cost[2 * blockIdx.x] = 0.0; tile_cost[2 * blockIdx.x + 1] = 0.0; }
        return;
    }
    if (act) {
        sRow[pos] = (unsigned short)(run_id[s] - row_first);
        sSrc[pos] = (unsigned short)tid;
    }
    // the tile's objective, added in a fixed order; its count stays 0: cost_count[1] counts samples
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) obj += __shfl_xor(obj, o, 64);
    if (lane == 0) sObj[wv] = obj;
    __syncthreads();
    if (tid == 0) {
        double o = sObj[0];
#pragma unroll
        for (int w_ = 1; w_ < kLmWaves; ++w_) o += sObj[w_];
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
            for (int w_ = 0; w_ < kLmWaves; ++w_) n += sWaveCnt[w_];
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
    // Gram matrix of every run, G = X^T X with X = the run's rows of [J_a | r_a] (3 n x (6K + 1)), on the matrix cores as 16 x 16
    // tiles of v_mfma_f64_16x16x4_f64: one wave per run, runs dealt round-robin by their index in the tile.
    constexpr int NC = NJ + 1;
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
    for (int c0 = 0; c0 < n_valid; c0 += CH) {
        const int c1 = min(n_valid, c0 + CH);
        if (c0 > 0) __syncthreads();                                 // the previous pass' rows have been read
        const int ci = tid / 3, a = tid - 3 * ci;
        if (tid < 3 * CH && c0 + ci < c1) {
            LandmarkState st;
            landmark_state<K>(blockIdx.x * kTile + sSrc[c0 + ci], lpos, nbr, wts, target, valid, conf, node_dq, p, st);
            double Jrow[NJ];
            landmark_axis_row(node_dq, st.idx, st.w, K, p.lw.q, st.bh, st.nb, st.pf[0], st.pf[1], st.pf[2], a, st.sc, Jrow);
#pragma unroll
            for (int j = 0; j < NJ; ++j) sJ[tid * LD + j] = Jrow[j];
            sJ[tid * LD + NJ] = st.sc * (a == 0 ? st.d[0] : (a == 1 ? st.d[1] : st.d[2]));
        }
        __syncthreads();
        for (int rn = wv; rn < n_runs; rn += kLmWaves) {
            const int t0 = sRun[rn], t1 = sRun[rn + 1];
            if (t1 <= c0 || t0 >= c1) continue;                      // (wave-uniform) no landmark of this run in this pass
            const int r0 = 3 * (max(t0, c0) - c0), r1 = 3 * (min(t1, c1) - c0);      // its rows in sJ
            const bool carry = t0 < c0, last = t1 <= c1;             // begun in an earlier pass / complete with this one
            double *dst = partial + (size_t)(row_first + sRow[t0]) * ST_;
            d4 acc[NT * (NT + 1) / 2];
            {
                int q = 0;
#pragma unroll
                for (int bi = 0; bi < NT; ++bi)
#pragma unroll
                    for (int bj = bi; bj < NT; ++bj, ++q)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {                // C/D: column = lane & 15, row = (lane >> 4) + 4 r
                            const int i = slot(16 * bi + lk + 4 * r, 16 * bj + li);
                            acc[q][r] = (carry && i >= 0) ? dst[i] : 0.0;
                        }
            }
            for (int t = r0; t < r1; t += 4) {
                double x[NT];                                        // A[i = li][k = lk] = B[k = lk][j = li] = X[t + lk][16 b + li]
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
                            // a diagonal sub-block that straddles two tiles: its lower entries lie in the tile that is not
                            // computed; the product is symmetric bit for bit
                            if (last && bi != bj && pb < NJ && pa / 6 == pb / 6)
                                dst[36 * gn_sub(K, pa / 6, pa / 6) + 6 * (pb - 6 * (pb / 6)) + (pa - 6 * (pa / 6))] = v;
                        }
                    }
        }
    }
}

int gn_add_landmarks_impl(const dfh_gn_problem &q, const dfh_gn_landmarks &l, void *stream) {
    if (l.n == 0 || l.weight == 0.0) return DFH_OK;                  // nothing to add: no launch, the system stays as it is
    hipStream_t s = (hipStream_t)stream;
    const int n_tiles = (l.n + kTile - 1) / kTile;
    LandmarkParams p;
    for (int i = 0; i < 8; ++i) p.lw.q[i] = q.lw_dq[i];
    p.n = l.n; p.weight = l.weight; p.huber = l.huber_delta; p.max_dist = l.max_dist;
    double *tile_cost = l.partial + (size_t)l.n_rows * gn_row_stride(q.knn);      // 2 doubles per tile, then one live flag per row
    dim3 grid((unsigned)n_tiles), block(kLmThreads);
#define DFH_LANDMARKS(KK)                                                                                           \
    case KK:                                                                                                        \
        hipLaunchKernelGGL(gn_landmark_rows_kernel<KK>, grid, block, 0, s, l.pos, l.nbr, l.weights, l.target, l.valid, l.conf, q.node_dq, p, \
                           l.run_id, l.partial, tile_cost, n_tiles, l.active_out);                                   \
        break
    switch (q.knn) {
        DFH_LANDMARKS(1); DFH_LANDMARKS(2); DFH_LANDMARKS(3); DFH_LANDMARKS(4); DFH_LANDMARKS(5); DFH_LANDMARKS(6); DFH_LANDMARKS(7); DFH_LANDMARKS(8);
    }
#undef DFH_LANDMARKS
    DFH_HIP_CHECK(hipGetLastError());
    const int *upper = (q.blk_upper && q.n_upper > 0 && !on(opt().gn_gather_full)) ? q.blk_upper : nullptr;
    return gn_gather_launch(q.knn, l.partial, tile_cost + 2 * (size_t)n_tiles, l.n_rows, l.blk_ptr, l.blk_ent, q.n_blocks, l.node_ptr,
                            l.node_ent, q.n_nodes, q.vals, q.rhs, q.cost_count, tile_cost, n_tiles, true, upper, q.n_upper, stream);
}

}  // namespace dfh

extern "C" {

int dfh_gn_add_landmarks(const dfh_gn_problem *problem, const dfh_gn_landmarks *landmarks, void *stream) {
    using namespace dfh;
    int rc = check_problem("dfh_gn_add_landmarks", problem, true);
    if (rc == DFH_OK) rc = check_landmarks("dfh_gn_add_landmarks", landmarks);
    if (rc != DFH_OK) return rc;
    return gn_add_landmarks_impl(*problem, *landmarks, stream);
}

}  // extern "C"
