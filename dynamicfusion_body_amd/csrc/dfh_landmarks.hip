// K16: the landmark term of the warp-field solve -- point-to-point rows for feature correspondences (include/dfusion_hip.h:
// dfh_gn_landmarks; restated in tests/landmark_np.py).
//
// A landmark is a canonical point with a live 3-D target: three rows sc (x' - c)_a, a = 0, 1, 2, where the data term has the one
// row n'.(x' - c).  The rows go the way of every sparse term (dfh_gn_term_rows.h: tiles of kTile landmarks sorted by node tuple, a
// scratch row per run, its Gram matrix stored there, the gather with accumulate = true).
//
// A run's rows are 3 n x (6K + 1): three times the data term's LDS if staged whole (150 KB at K = 8).  The tile's active landmarks
// are therefore staged kTile / 3 at a time, each with its three axis rows side by side: pass c holds the rows of compacted
// landmarks [CH c, CH c + CH), CH = kTile / 3, one (landmark, axis) pair per thread -- the pair's thread warps the landmark again (the same
// functions on the same values as the gate's pass: the same bits) and differentiates its axis.  A run's accumulators take its rows
// in the fixed order landmark by landmark, axis 0, 1, 2.  A run that a pass boundary cuts (at most one per boundary) is carried
// through its scratch row (gram_run's carry); the run belongs to one wave in every pass.
#include "dfh_gn_term_rows.h"

#include <cmath>

namespace dfh {

struct LandmarkParams {
    DQ lw;
    int n;
    double weight, huber, max_dist;
};

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
    if (st.act) robust_scale(q, s2, p.huber, st.obj, st.sc);         // vector Huber on |d|
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
    constexpr int CH = kTile / 3;               // landmarks per pass: 3 CH rows, one per thread
    __shared__ double sJ[3 * CH * LD];          // one pass' rows: compacted landmark c0 + i, axis a in row 3 i + a
    __shared__ TermTile<kLmWaves> sT;
    __shared__ unsigned short sSrc[kTile];      // the thread (= landmark of the tile) every compacted landmark came from
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
    int pos, n_valid, row_first, rows_tile;
    if (!term_tile_compact(sT, act, run_id, tile_n, tile_cost, n_tiles, pos, n_valid, row_first, rows_tile)) return;
    if (act) {
        sT.row[pos] = (unsigned short)(run_id[s] - row_first);
        sSrc[pos] = (unsigned short)tid;
    }
    const int n_runs = term_tile_runs<K>(sT, obj, n_valid, row_first, rows_tile, partial, tile_cost, n_tiles);
    // Gram matrix of every run over X = the run's rows of [J_a | r_a] (3 n x (6K + 1)): one wave per run, runs dealt round-robin by
    // their index in the tile.
    for (int c0 = 0; c0 < n_valid; c0 += CH) {
        const int c1 = min(n_valid, c0 + CH);
        if (c0 > 0) __syncthreads();                                 // the previous pass' rows have been read
        const int ci = tid / 3, a = tid - 3 * ci;
        if (tid < 3 * CH && c0 + ci < c1) {
            LandmarkState st;
            landmark_state<K>(blockIdx.x * kTile + sSrc[c0 + ci], lpos, nbr, wts, target, valid, conf, node_dq, p, st);
            const double e[3] = {a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0};
            double Jrow[NJ];
            point_row(node_dq, st.idx, st.w, K, p.lw.q, st.bh, st.nb, st.pf[0], st.pf[1], st.pf[2], e, st.sc, Jrow);
#pragma unroll
            for (int j = 0; j < NJ; ++j) sJ[tid * LD + j] = Jrow[j];
            sJ[tid * LD + NJ] = st.sc * (a == 0 ? st.d[0] : (a == 1 ? st.d[1] : st.d[2]));
        }
        __syncthreads();
        for (int rn = wv; rn < n_runs; rn += kLmWaves) {
            const int t0 = sT.run[rn], t1 = sT.run[rn + 1];
            if (t1 <= c0 || t0 >= c1) continue;                      // (wave-uniform) no landmark of this run in this pass
            // its rows in sJ; begun in an earlier pass / complete with this one
            gram_run<K, true>(sJ, 3 * (max(t0, c0) - c0), 3 * (min(t1, c1) - c0), t0 < c0, t1 <= c1,
                              partial + (size_t)(row_first + sT.row[t0]) * gn_row_stride(K), lane);
        }
    }
}

int gn_add_landmarks_impl(const dfh_gn_problem &q, const dfh_gn_landmarks &l, void *stream) {
    if (l.n == 0 || l.weight == 0.0) return DFH_OK;                  // nothing to add: no launch, the system stays as it is
    LandmarkParams p;
    for (int i = 0; i < 8; ++i) p.lw.q[i] = q.lw_dq[i];
    p.n = l.n; p.weight = l.weight; p.huber = l.huber_delta; p.max_dist = l.max_dist;
    return term_add(q, term_plan(l), l.n, stream, [&](auto kk, dim3 grid, double *tile_cost, int n_tiles) {
        hipLaunchKernelGGL(gn_landmark_rows_kernel<decltype(kk)::value>, grid, dim3(kLmThreads), 0, (hipStream_t)stream, l.pos, l.nbr,
                           l.weights, l.target, l.valid, l.conf, q.node_dq, p, l.run_id, l.partial, tile_cost, n_tiles, l.active_out);
    });
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
