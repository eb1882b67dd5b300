// Normal equations of the warp-field solve, and the Gauss-Newton iteration around them.
//
// The reference has no Gauss-Newton: it calls scipy's trust-region solver with finite-difference Jacobians
// (core/fusion.py:382-392).  Here: projective data association against the frame's views (dfh_gn_rows.h), analytic
// Jacobian rows, and J^T J / J^T r in 6x6 block-sparse rows.  Samples arrive sorted by their k-node tuple, one kTile-sample
// tile per workgroup.  The planned build -- what ships -- has no floating-point atomics: the (tile, tuple) runs are static
// per frame (dfh_plan.hip), each run's Gram matrix is accumulated with v_mfma_f64_16x16x4 and STORED in a scratch row of
// its own, and gn_gather_kernel adds the rows into the blocks through a precomputed incidence list -- the same bits every
// run.  Without a plan the sums reach the blocks by one fp64 atomic per entry and run.
//
// Everything is fp64: per GN iteration the work is ~1 kflop/sample over ~1e5..1e6 samples, far from any roofline that
// would justify fp32, and fp64 keeps the residual bit-comparable with the CPU path.
#include "dfh_assoc_volume.h"
#include "dfh_gn_rows.h"
#include "dfh_pcg.h"

#include <cmath>
#include <cstring>

namespace dfh {

// Warp every sample with the current field, project it into the live depth frame with the
// reference's primitives and back-project the nearest depth pixel: corr (index space), valid.
template <typename DepthT>
__global__ __launch_bounds__(256) void associate_kernel(const double *__restrict__ spos, const int *__restrict__ nbr,
                                                         const double *__restrict__ wts, int S,
                                                         const double *__restrict__ node_dq,
                                                         const AssocParams p, double *__restrict__ corr,
                                                         unsigned char *__restrict__ valid, const AssocView *__restrict__ views, int n_views) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    int idx[kKMaxS];
    double w[kKMaxS];
#pragma unroll
    for (int j = 0; j < kKMaxS; ++j) {
        idx[j] = j < p.k ? nbr[(size_t)i * p.k + j] : 0;
        w[j] = j < p.k ? wts[(size_t)i * p.k + j] : 0.0;
    }
    double b[8];
    blend_static(node_dq, idx, w, p.k, b);
    const double px = spos[3 * (size_t)i], py = spos[3 * (size_t)i + 1], pz = spos[3 * (size_t)i + 2];
    const D3 x1 = dqb_warp_exact(b, round_f32(px), round_f32(py), round_f32(pz));
    const D3 xp = dqb_warp_exact(p.lw.q, round_f32(x1.x), round_f32(x1.y), round_f32(x1.z));
    double c[3];
    const bool ok = associate_views<DepthT>(p, views, n_views, xp, c);
    corr[3 * (size_t)i] = c[0];
    corr[3 * (size_t)i + 1] = c[1];
    corr[3 * (size_t)i + 2] = c[2];
    valid[i] = ok ? 1 : 0;
}

// associate_kernel through the normal gate (dfh_gn_associate_gated): the sample's warped normal first -- data_row_from's n', the
// same bits -- then the association with the live normals beside the depth values.
template <typename DepthT>
__global__ __launch_bounds__(256) void associate_gated_kernel(const double *__restrict__ spos, const double *__restrict__ snrm,
                                                               const int *__restrict__ nbr, const double *__restrict__ wts, int S,
                                                               const double *__restrict__ node_dq, const AssocParams p,
                                                               double *__restrict__ corr, unsigned char *__restrict__ valid,
                                                               const AssocView *__restrict__ views, int n_views, const NormalGate ng) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    int idx[kKMaxS];
    double w[kKMaxS];
#pragma unroll
    for (int j = 0; j < kKMaxS; ++j) {
        idx[j] = j < p.k ? nbr[(size_t)i * p.k + j] : 0;
        w[j] = j < p.k ? wts[(size_t)i * p.k + j] : 0.0;
    }
    double b[8];
    blend_static(node_dq, idx, w, p.k, b);
    const double px = spos[3 * (size_t)i], py = spos[3 * (size_t)i + 1], pz = spos[3 * (size_t)i + 2];
    const D3 x1 = dqb_warp_exact(b, round_f32(px), round_f32(py), round_f32(pz));
    const D3 xp = dqb_warp_exact(p.lw.q, round_f32(x1.x), round_f32(x1.y), round_f32(x1.z));
    const D3 np_ = warped_normal(b, p.lw.q, snrm[3 * (size_t)i], snrm[3 * (size_t)i + 1], snrm[3 * (size_t)i + 2]);
    double c[3];
    const bool ok = associate_views<DepthT, true>(p, views, n_views, xp, c, ~0u, ng.normals, ng.min_cos, np_.x, np_.y, np_.z);
    corr[3 * (size_t)i] = c[0];
    corr[3 * (size_t)i + 1] = c[1];
    corr[3 * (size_t)i + 2] = c[2];
    valid[i] = ok ? 1 : 0;
}

// ------------------------------------------------------------------------------- normal equations
// One kTile-sample tile per block.  Samples must be sorted by their k-tuple of nodes (any order
// is CORRECT; sorted order just means few runs per tile and therefore few atomics).
// PLANNED: the (tile, tuple) runs are static per frame, so each run owns a row of `partial`
// ({upper triangle of its (6K)^2 Gram matrix | J^T r | 0.5 r^2 | count}, row = run_id[first sample]) and the
// sums are STORED there; gn_gather_kernel then adds the rows into the blocks through a precomputed incidence
// list: no floating-point atomics, same bits every run, about half the memory operations.
// The regulariser's pair rows (gn_reg_pairs, below) are independent of the data rows: in the planned build they are
// computed by extra workgroups appended to the data-row launch (blockIdx.x >= n_tiles) instead of a launch of their own.
struct RegTail {
    const int *node_nbr;        // NULL: no regulariser workgroups
    const double *node_pos, *node_w;
    double *partial_reg;
    double rw;
    int N, k, n_tiles;
    // dfh_gn_solve: doubles the launch's LAST workgroups set to zero (the solve's workspace: its clearing rides along here
    // instead of being a launch of its own between gather and solve); first_zero_wg = index of the first such workgroup
    double *zero_ptr;
    unsigned long long zero_count;
    int first_zero_wg;
};
constexpr int kZeroPerWg = 4 * kTile;            // doubles one workgroup clears (kTile threads x 4)
__device__ void gn_reg_pairs(int block, const int *__restrict__ node_nbr, int N, int k, const double *__restrict__ node_dq,
                             const double *__restrict__ node_pos, const double *__restrict__ node_w, double rw,
                             const int *__restrict__ row_ptr, const int *__restrict__ col, double *__restrict__ vals,
                             double *__restrict__ rhs, double *__restrict__ cost_count, double *__restrict__ partial_reg);

// MODE != AssocMode::None: the association runs inside this kernel -- every sample of the tile is warped once, associated, its
// correspondence and validity are written to corr / valid (for the callers that read them) and the valid ones go straight on to
// their Jacobian rows: one launch and one blend + warp per sample less per GN iteration.  Views: the projective association
// against the frame's views (associate_kernel's arithmetic, same bits).  Volume: one trilinear cell of a live TSDF volume
// (associate_volume_kernel's arithmetic, same bits: dfh_assoc_volume.h) -- no views, so no tile box and no view mask.
// The kernel's last argument is what its mode reads: the views' arguments (also for None, which reads nothing: its kernarg
// segment is what it was), or the volume's.  ViewsGated: Views through the normal gate (dfh_gn_rows.h: associate_views<.., true>) --
// the sample's warped normal is computed in front of the association, and the gate's arguments travel in a struct of this mode's
// own, so the other modes get no new kernel argument.
enum class AssocMode { None, Views, Volume, ViewsGated };
template <AssocMode MODE> struct AssocArgsOf { typedef AssocArgs type; };
template <> struct AssocArgsOf<AssocMode::Volume> { typedef VolAssocArgs type; };
template <> struct AssocArgsOf<AssocMode::ViewsGated> { typedef GatedAssocArgs type; };
#ifdef DFH_BUILD_TRACE   // experiment builds only: wall-clock stamps of every tile's phases
__device__ unsigned long long g_build_trace[8192][8];
#define BT_STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < 8192) g_build_trace[blockIdx.x][k] = wall_clock64(); } while (0)
#else
#define BT_STAMP(k) do {} while (0)
#endif

template <int K, bool PLANNED, AssocMode MODE>
__global__ __launch_bounds__(kTile) void gn_build_data_kernel(const double *__restrict__ spos, const double *__restrict__ snrm,
                                                             const int *__restrict__ nbr, const double *__restrict__ wts,
                                                             double *__restrict__ corr,
                                                             unsigned char *__restrict__ valid,
                                                             const double *__restrict__ node_dq, const BuildParams p,
                                                             const int *__restrict__ row_ptr, const int *__restrict__ col,
                                                             double *__restrict__ vals, double *__restrict__ rhs,
                                                             double *__restrict__ cost_count, const int *__restrict__ run_id,
                                                             double *__restrict__ partial, double *__restrict__ tile_cost,
                                                             const RegTail rt, const typename AssocArgsOf<MODE>::type aa) {
    constexpr bool ASSOC = MODE != AssocMode::None;
    if (PLANNED && rt.zero_ptr && (int)blockIdx.x >= rt.first_zero_wg) {     // (workgroup-uniform) clearing that rides along
        const unsigned long long i0 = (unsigned long long)((int)blockIdx.x - rt.first_zero_wg) * kZeroPerWg + 4ull * threadIdx.x;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < rt.zero_count) rt.zero_ptr[i0 + j] = 0.0;
        return;
    }
    if (PLANNED && (int)blockIdx.x >= rt.n_tiles) {      // (workgroup-uniform) the regulariser's share of this launch
        gn_reg_pairs((int)blockIdx.x - rt.n_tiles, rt.node_nbr, rt.N, rt.k, node_dq, rt.node_pos, rt.node_w, rt.rw, row_ptr, col, vals,
                     rhs, cost_count, rt.partial_reg);
        return;
    }
    BT_STAMP(0);
    constexpr int NJ = 6 * K;                   // Jacobian entries per sample
    constexpr int LD = NJ + 1;                  // + residual
    __shared__ double sJ[kTile * LD];
    // (the planned build tells runs apart by their scratch-row ids and needs no node tuples in LDS; without them and with 16-bit
    // row ids the workgroup's LDS drops from 58.4 to 52.8 KB: three workgroups per CU instead of two)
    __shared__ int sIdx[PLANNED ? 1 : kTile * K];
    const int tid = threadIdx.x;
    const int s = blockIdx.x * kTile + tid;
    const int tile_n = min(kTile, p.S - blockIdx.x * kTile);
    // ---- each valid sample computes its residual and Jacobian row and appends it to the tile's
    // compacted list in LDS (order preserved): the reduction below only walks valid rows
    int idx[kKMaxS];
    double w[kKMaxS];
    double a_bh[8], a_nb = 1.0, a_pf[3] = {0, 0, 0}, a_c[3] = {0, 0, 0};
    D3 a_xp{0, 0, 0};
    bool a_ok = false;
    // the sample's normal is only needed for its Jacobian row, but asking for it here takes a memory round trip out of that phase
    double a_n[3] = {0.0, 0.0, 0.0};
    if (ASSOC && tid < tile_n) {
        a_n[0] = snrm[3 * (size_t)s]; a_n[1] = snrm[3 * (size_t)s + 1]; a_n[2] = snrm[3 * (size_t)s + 2];
    }
    if (ASSOC && tid < tile_n) {
#pragma unroll
        for (int j = 0; j < kKMaxS; ++j) {
            idx[j] = j < K ? nbr[(size_t)s * K + j] : 0;
            w[j] = j < K ? wts[(size_t)s * K + j] : 0.0;
        }
        a_nb = blend_static(node_dq, idx, w, K, a_bh);
        a_pf[0] = round_f32(spos[3 * (size_t)s]); a_pf[1] = round_f32(spos[3 * (size_t)s + 1]); a_pf[2] = round_f32(spos[3 * (size_t)s + 2]);
        const D3 x1 = dqb_warp_exact(a_bh, a_pf[0], a_pf[1], a_pf[2]);
        a_xp = dqb_warp_exact(p.lw.q, round_f32(x1.x), round_f32(x1.y), round_f32(x1.z));
    }
    if constexpr (MODE == AssocMode::Views || MODE == AssocMode::ViewsGated) {
        unsigned view_mask = ~0u;
        if (aa.views && aa.cull) {                                            // (workgroup-uniform)
            // the tile's warped samples' box -> the views any of them can be valid in
            __shared__ double sBox[kTileWaves][6];
            __shared__ unsigned sMask;
            const bool in = tid < tile_n;
            double bx[6] = {in ? a_xp.x : __builtin_huge_val(), in ? -a_xp.x : __builtin_huge_val(), in ? a_xp.y : __builtin_huge_val(),
                            in ? -a_xp.y : __builtin_huge_val(), in ? a_xp.z : __builtin_huge_val(), in ? -a_xp.z : __builtin_huge_val()};
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
#pragma unroll
                for (int c6 = 0; c6 < 6; ++c6) bx[c6] = fmin(bx[c6], __shfl_xor(bx[c6], o, 64));
            if ((tid & 63) == 0)
#pragma unroll
                for (int c6 = 0; c6 < 6; ++c6) sBox[tid >> 6][c6] = bx[c6];
            __syncthreads();
            double box[6];
#pragma unroll
            for (int c6 = 0; c6 < 6; ++c6) {
                double m = sBox[0][c6];
#pragma unroll
                for (int w_ = 1; w_ < kTileWaves; ++w_) m = fmin(m, sBox[w_][c6]);
                box[c6] = (c6 & 1) ? -m : m;                                       // (maxima were carried negated)
            }
            view_mask = tile_view_mask(aa.ap, aa.views, aa.n_views, box, &sMask);
        }
        if constexpr (MODE == AssocMode::ViewsGated) {
            // (n' before the association; data_row_from arrives at the same bits afterwards -- the same inlined functions on the same
            // values, so whether the registers are kept or the normal is warped again is the compiler's choice)
            if (tid < tile_n) {
                const D3 a_np = warped_normal(a_bh, p.lw.q, a_n[0], a_n[1], a_n[2]);
                a_ok = associate_views<float, true>(aa.ap, aa.views, aa.n_views, a_xp, a_c, view_mask, aa.ng.normals, aa.ng.min_cos, a_np.x, a_np.y, a_np.z);
            }
        } else {
            if (tid < tile_n)
                a_ok = associate_views<float>(aa.ap, aa.views, aa.n_views, a_xp, a_c, view_mask);
        }
    } else if constexpr (MODE == AssocMode::Volume) {
        // (lanes beyond the ragged last tile hold no sample: they issue no live-volume load)
        if (tid < tile_n) a_ok = associate_volume_cell<float>(static_cast<const float *>(aa.live), aa.vp, a_xp, a_c);
    }
    // corr / valid are outputs only: stored after the last global load of the kernel (stored here, every later s_waitcnt for a
    // load also waited for these stores' acknowledgements)
    auto store_assoc = [&]() {
        if (ASSOC && tid < tile_n) {
            corr[3 * (size_t)s] = a_c[0]; corr[3 * (size_t)s + 1] = a_c[1]; corr[3 * (size_t)s + 2] = a_c[2];
            valid[s] = a_ok ? 1 : 0;
        }
    };
    const bool act = ASSOC ? a_ok : (tid < tile_n && valid[s] != 0);
    BT_STAMP(1);
    __shared__ int sWaveCnt[kTileWaves];
    const unsigned long long bal = __ballot(act);
    const int lane = tid & 63, wv = tid >> 6;
    if (lane == 0) sWaveCnt[wv] = __popcll(bal);
    __syncthreads();
    int pos = __popcll(bal & ((1ull << lane) - 1ull));
    for (int w_ = 0; w_ < wv; ++w_) pos += sWaveCnt[w_];
    int n_valid = 0;
#pragma unroll
    for (int w_ = 0; w_ < kTileWaves; ++w_) n_valid += sWaveCnt[w_];
    constexpr int ST_ = gn_row_stride(K);
    double *live = PLANNED ? tile_cost + 2 * (size_t)rt.n_tiles : nullptr;      // one flag per row, dense: 0 = row not written this iteration
    const int row_first = PLANNED ? run_id[blockIdx.x * kTile] : 0;
    const int rows_tile = PLANNED ? run_id[blockIdx.x * kTile + tile_n - 1] - row_first + 1 : 0;
    if (n_valid == 0) {                                              // tiles without a valid sample contribute nothing:
        store_assoc();
        if (PLANNED && tid < rows_tile) live[row_first + tid] = 0.0;                                 // their rows are dead
        if (PLANNED && tid == 0) { tile_cost[2 * blockIdx.x] = 0.0; tile_cost[2 * blockIdx.x + 1] = 0.0; }
        return;
    }
    if (!PLANNED && tid == 0) atomicAdd(cost_count + 1, (double)n_valid);        // valid-sample count
    __shared__ unsigned short sRow[PLANNED ? kTile : 1];             // partial row of every compacted sample, relative to the tile's first
    __shared__ double sObj[kTileWaves];
    double obj = 0.0;
    if (act) {
        if (PLANNED) sRow[pos] = (unsigned short)(run_id[s] - row_first);
        double Jrow[NJ];
        double r;
        if (ASSOC) {
            r = data_row_from(node_dq, idx, w, K, p.lw.q, a_bh, a_nb, a_pf[0], a_pf[1], a_pf[2], a_xp, a_n[0], a_n[1], a_n[2], a_c[0], a_c[1],
                              a_c[2], Jrow);
        } else {
#pragma unroll
            for (int j = 0; j < kKMaxS; ++j) {
                idx[j] = j < K ? nbr[(size_t)s * K + j] : 0;
                w[j] = j < K ? wts[(size_t)s * K + j] : 0.0;
            }
            r = data_row(node_dq, idx, w, K, p.lw.q, spos[3 * (size_t)s], spos[3 * (size_t)s + 1], spos[3 * (size_t)s + 2],
                         snrm[3 * (size_t)s], snrm[3 * (size_t)s + 1], snrm[3 * (size_t)s + 2], corr[3 * (size_t)s],
                         corr[3 * (size_t)s + 1], corr[3 * (size_t)s + 2], Jrow);
        }
        obj = 0.5 * r * r;                                     // this sample's term of the objective
        if (p.huber > 0.0 && fabs(r) > p.huber) {              // Huber: rho = delta (|r| - delta / 2) beyond delta, and the
            obj = p.huber * (fabs(r) - 0.5 * p.huber);         // row and its residual get sqrt of the IRLS weight
            const double sc = sqrt(p.huber / fabs(r));
            r *= sc;
#pragma unroll
            for (int j = 0; j < NJ; ++j) Jrow[j] *= sc;
        }
        if (!PLANNED) {
#pragma unroll
            for (int j = 0; j < K; ++j) sIdx[pos * K + j] = idx[j];
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) sJ[pos * LD + j] = Jrow[j];
        sJ[pos * LD + NJ] = r;
    }
    store_assoc();
    BT_STAMP(2);
    if (PLANNED) {                                                   // the tile's objective, added in a fixed order
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) obj += __shfl_xor(obj, o, 64);
        if (lane == 0) sObj[wv] = obj;
    }
    __syncthreads();
    if (PLANNED && tid == 0) {
        double o = sObj[0];                                          // (fixed order)
#pragma unroll
        for (int w_ = 1; w_ < kTileWaves; ++w_) o += sObj[w_];
        tile_cost[2 * blockIdx.x] = o;
        tile_cost[2 * blockIdx.x + 1] = (double)n_valid;
    }
    // run boundaries: sRun[0..n_runs] are the offsets in the compacted list where the node tuple changes
    __shared__ int sRun[kTile + 1];
    __shared__ int sNRuns;
    {
        bool head = false;
        if (tid < n_valid) {
            head = tid == 0;
            if (!head) {
                if (PLANNED) {
                    head = sRow[tid] != sRow[tid - 1];               // (a scratch row = a run of equal tuples inside the tile)
                } else {
#pragma unroll
                    for (int j = 0; j < K; ++j) head = head || (sIdx[tid * K + j] != sIdx[(tid - 1) * K + j]);
                }
            }
        }
        // positions of the heads by ballot + prefix (same scheme as the compaction above)
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
        __syncthreads();
    }
    const int n_runs = sNRuns;
    BT_STAMP(3);
#ifdef DFH_BUILD_TRACE
    if (threadIdx.x == 0 && blockIdx.x < 8192) g_build_trace[blockIdx.x][6] = (unsigned long long)n_valid | ((unsigned long long)n_runs << 16);
#endif
    // block index of every (slot a, slot b) node pair of every run, searched once, in parallel
    constexpr bool kBlkTable = K <= 4 && !PLANNED;         // 256 runs x K^2 ints must fit next to sJ
    __shared__ int sBlk[kBlkTable ? kTile * K * K : 1];
    if (kBlkTable) {
        for (int q = tid; q < n_runs * K * K; q += kTile) {
            const int rn = q / (K * K), pr = q - rn * (K * K);
            const int t0 = sRun[rn];
            sBlk[q] = find_block(row_ptr, col, sIdx[t0 * K + pr / K], sIdx[t0 * K + pr % K]);
        }
        __syncthreads();
    }
    // entries: PLANNED: the 6x6 sub-blocks (sa <= sb) of the Gram matrix in scratch-row order; else its upper triangle; then NJ
    // entries of J^T r, then the cost
    constexpr int NUP = PLANNED ? gn_row_gram(K) : NJ * (NJ + 1) / 2;
    if (PLANNED) {
        if (tid < n_runs) partial[(size_t)(row_first + sRow[sRun[tid]]) * ST_ + NUP + NJ + 1] = (double)(sRun[tid + 1] - sRun[tid]);
        // live flags of this tile's rows: 1 where a run has valid samples this iteration, 0 elsewhere (dead rows are
        // neither cleared here nor read by the gather)
        __shared__ int sTouched[kTile];
        if (tid < rows_tile) sTouched[tid] = 0;
        __syncthreads();
        if (tid < n_runs) sTouched[sRow[sRun[tid]]] = 1;
        __syncthreads();
        if (tid < rows_tile) live[row_first + tid] = sTouched[tid] ? 1.0 : 0.0;
    }
    BT_STAMP(4);
    if constexpr (PLANNED) {
        // Gram matrix of every run on the matrix cores: G = X^T X with X = the run's rows of [J | r] (n x (6K + 1)), as 16 x 16
        // tiles of v_mfma_f64_16x16x4_f64 (four samples per step, A and B fragments straight from the compacted rows in
        // LDS: two reads per lane and step where the scalar loop read two values per sample and ENTRY).  One wave per
        // run, runs dealt round-robin; the accumulation order (sample order, fused multiply-add) is fixed, so the bits are
        // the same every launch.  Each lane then stores its accumulator elements straight to their places in the scratch
        // row (a 16-lane group writes three 48-byte runs; the row is written whole by this wave).
        constexpr int NC = NJ + 1;                                   // columns: Jacobian + residual
        constexpr int NT = (NC + 15) / 16;                           // 16-column tiles per side
        typedef double d4 __attribute__((ext_vector_type(4)));
        const int li = lane & 15, lk = lane >> 4;
        for (int rn = wv; rn < n_runs; rn += kTile / 64) {
            const int t0 = sRun[rn], t1 = sRun[rn + 1];
            d4 acc[NT * (NT + 1) / 2];
#pragma unroll
            for (int q = 0; q < NT * (NT + 1) / 2; ++q) acc[q] = d4{0.0, 0.0, 0.0, 0.0};
            for (int t = t0; t < t1; t += 4) {
                double x[NT];                                        // A[i = li][k = lk] = B[k = lk][j = li] = X[t + lk][16 b + li]
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
                    for (int r = 0; r < 4; ++r) {                    // C/D: column = lane & 15, row = (lane >> 4) + 4 r
                        const int pa = 16 * bi + lk + 4 * r, pb = 16 * bj + li;
                        const double v = acc[q][r];
                        if (pa < NJ && pb < NJ) {
                            const int sa = pa / 6, sb = pb / 6;
                            if (sa <= sb) {
                                dst[36 * gn_sub(K, sa, sb) + 6 * (pa - 6 * sa) + (pb - 6 * sb)] = v;
                                // a diagonal sub-block that straddles two tiles: its lower entries lie in the tile that is
                                // not computed; the product is symmetric bit for bit
                                if (bi != bj && sa == sb) dst[36 * gn_sub(K, sa, sa) + 6 * (pb - 6 * sb) + (pa - 6 * sa)] = v;
                            }
                        } else if (pa < NJ && pb == NJ) {
                            dst[NUP + pa] = v;                       // J^T r
                        } else if (pa == NJ && pb == NJ) {
                            dst[NUP + NJ] = 0.5 * v;                 // cost
                        }
                    }
        }
        BT_STAMP(5);
        return;
    }
    for (int e = tid; e < NUP + NJ + 1; e += kTile) {
        int pa, pb;                              // Jacobian columns of this entry (pb == NJ: residual)
        if (e < NUP && PLANNED) {
            int sub = e / 36, sa = 0;
            const int r36 = e - 36 * sub;
            while (sub >= K - sa) { sub -= K - sa; ++sa; }          // sub-block (sa, sa + sub)
            pa = 6 * sa + r36 / 6; pb = 6 * (sa + sub) + r36 % 6;   // (a diagonal sub-block's lower entries: same products, same order)
        } else if (e < NUP) {
            int row = 0, rem = e;
            while (rem >= NJ - row) { rem -= NJ - row; ++row; }
            pa = row; pb = row + rem;
        } else if (e < NUP + NJ) {
            pa = e - NUP; pb = NJ;
        } else {
            pa = NJ; pb = NJ;
        }
        for (int rn = 0; rn < n_runs; ++rn) {
            const int t0 = sRun[rn], t1 = sRun[rn + 1];
            // four independent chains: the loop is bound by LDS latency, not bandwidth (fixed association order)
            double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
            int t = t0;
            for (; t + 3 < t1; t += 4) {
                const double a0 = sJ[t * LD + pa], b0 = sJ[t * LD + pb];
                const double a1 = sJ[(t + 1) * LD + pa], b1 = sJ[(t + 1) * LD + pb];
                const double a2 = sJ[(t + 2) * LD + pa], b2 = sJ[(t + 2) * LD + pb];
                const double a3 = sJ[(t + 3) * LD + pa], b3 = sJ[(t + 3) * LD + pb];
                acc0 += a0 * b0; acc1 += a1 * b1; acc2 += a2 * b2; acc3 += a3 * b3;
            }
            for (; t < t1; ++t) acc0 += sJ[t * LD + pa] * sJ[t * LD + pb];
            const double acc = (acc0 + acc1) + (acc2 + acc3);
            if (PLANNED) {
                partial[(size_t)(row_first + sRow[t0]) * ST_ + e] = pa == NJ ? 0.5 * acc : acc;
                continue;
            }
            if (acc == 0.0) continue;
            if (pb == NJ && pa == NJ) {
                atomicAdd(cost_count, 0.5 * acc);
            } else if (pb == NJ) {
                atomicAdd(rhs + 6 * sIdx[t0 * K + pa / 6] + pa % 6, acc);
            } else {
                const int sa = pa / 6, sb = pb / 6;
                const int na = sIdx[t0 * K + sa], nbn = sIdx[t0 * K + sb];
                const int ia = pa % 6, ib = pb % 6;
                const int blk = kBlkTable ? sBlk[rn * K * K + sa * K + sb] : find_block(row_ptr, col, na, nbn);
                if (blk >= 0) atomicAdd(vals + 36 * (size_t)blk + 6 * ia + ib, acc);
                if (!(na == nbn && ia == ib)) {
                    const int blk2 = na == nbn ? blk : (kBlkTable ? sBlk[rn * K * K + sb * K + sa] : find_block(row_ptr, col, nbn, na));
                    if (blk2 >= 0) atomicAdd(vals + 36 * (size_t)blk2 + 6 * ib + ia, acc);
                }
            }
        }
    }
    BT_STAMP(5);
}

// Second half of the planned build.  Workgroups [0, ceil(n_blocks/4)): one WAVE per 6x6 block (a,b), lanes 0..35 own
// entry (ia, ib) of the block and add the block's list (blk_ent = row * K^2 + sa * K + sb) in list order.  Next
// workgroups: J^T r, one wave per node, lane (j, i) takes every tenth entry of the node's list (node_ent = row * K +
// slot) for unknown i.  Last workgroup: cost and valid count, a fixed-order tree over the {cost, count} pairs.
// The regulariser's pair rows (K = 2 layout, own lists) are a second set of lists walked by the same wave right after
// the data rows': value = data sum + regulariser sum, the two roundings of "store, then add in a second launch".

// one wave: sum over block b's list of entry (ia, ib) of the rows' Gram matrices (lanes 0..35; others return 0)
template <int K>
__device__ __forceinline__ double gather_block_list(const double *__restrict__ partial, const double *__restrict__ live,
                                                    const int *__restrict__ blk_ptr, const int *__restrict__ blk_ent, int b, int lane,
                                                    int wv) {
    constexpr int NJ = 6 * K, NE = gn_row_stride(K), kLive = gn_row_entries(K);
    const int beg = blk_ptr[b], end = blk_ptr[b + 1];
    const int ia = (lane % 36) / 6, ib = lane % 6;
    auto value = [&](int ent) {
        const int row = ent / (K * K), pr = ent - row * (K * K);
        return partial[(size_t)row * NE + gn_gram_index(K, pr / K, pr % K, ia, ib)];
    };
    // The walk is a chain of dependent loads (entry -> live flag -> values), so it is organised by hops, not by
    // entries: up to 256 entries and then their flags are fetched together (two hops), the live ones are compacted
    // in list order into LDS, and lanes 0..35 (one per block entry) add them with 16 value loads in flight.
    __shared__ int sLiveB[4][256];
    double acc = 0.0;
    for (int base = beg; base < end; base += 256) {
        int ent[4];
        bool on[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) ent[u] = base + 64 * u + lane < end ? blk_ent[base + 64 * u + lane] : -1;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double flag = ent[u] >= 0 ? (live ? live[ent[u] / (K * K)] : partial[(size_t)(ent[u] / (K * K)) * NE + kLive]) : 0.0;
            on[u] = flag != 0.0;
        }
        int nl = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned long long m = __ballot(on[u]);
            if (on[u]) sLiveB[wv][nl + __popcll(m & ((1ull << lane) - 1ull))] = ent[u];
            nl += __popcll(m);
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < 36) {
            int q = 0;
            for (; q + 15 < nl; q += 16) {
                double v[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) v[u] = value(sLiveB[wv][q + u]);
#pragma unroll
                for (int u = 0; u < 16; ++u) acc += v[u];
            }
            for (; q + 3 < nl; q += 4) {
                double v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = value(sLiveB[wv][q + u]);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc += v[u];
            }
            for (; q < nl; ++q) acc += value(sLiveB[wv][q]);
        }
        __builtin_amdgcn_wave_barrier();
    }
    return acc;
}

#ifdef DFH_GATHER_TRACE  // experiment builds only: wall-clock stamps of every block wave's hops
__device__ unsigned long long g_gather_trace[8192][8];
#define GT_STAMP(k) do { __builtin_amdgcn_s_waitcnt(0); if (lane == 0 && b < 8192) g_gather_trace[b][k] = wall_clock64(); } while (0)
#else
#define GT_STAMP(k) do {} while (0)
#endif

// The data rows' list and the regulariser's list of one block walked TOGETHER: the walk is a chain of dependent hops (list
// bounds -> entries -> live flags -> values) and doing the two lists one after the other doubles the chain.  Here every
// hop is issued for both lists at once (4 hops).  Values are added in rounds of 16 loads in flight per lane (absent
// entries add 0.0).  A list with more than kCoopList live entries (the diagonal blocks: every row that touches the node,
// ~170) is split into four contiguous quarters, one per wave of the workgroup, and the quarters' sums are added in order
// -- walked by one wave alone it was eleven dependent rounds of ~2 us and set the whole launch's duration.
// Regulariser lists longer than 64 entries or data lists longer than 256 take the sequential walk.
#ifndef DFH_GATHER_DEPTH
#define DFH_GATHER_DEPTH 4
#endif
constexpr int kGatherDepth = DFH_GATHER_DEPTH;   // value loads in flight per lane and round
constexpr int kCoopList = 3 * kGatherDepth;

struct GatherLds {
    int liveD[4][256];
    int liveR[4][64];
    int coop[4];
    double part[4][4][36];
    double comb[4][3][2][36];
};

// lanes 0..35: sum of entry (ia, ib) = lane / 6, lane % 6 over list[q0, q1).  A list entry's sub-block is 36 contiguous
// doubles, so 18 lanes take it with one 16-byte load each and a load instruction covers THREE entries (lane group g takes
// entries q0 + g, q0 + g + 3, ...): kGatherDepth instructions in flight = 48 entries a round (a round costs ~3 us of
// latency whatever it carries).  Entries whose sub-block is stored transposed (tuple slots sa > sb) are added up in
// stored orientation on their own and transposed once at the end; the three groups' sums are added in group order.
// `comb` = this wave's scratch (3 x 2 x 36 doubles).  Order of the additions: fixed, not list order.
template <int K>
__device__ __forceinline__ double gather_rounds(const double *__restrict__ partial, const int *list, int q0, int q1, int lane,
                                                double (*comb)[2][36]) {
    constexpr int NE = gn_row_stride(K);
    const int g = lane / 18, h = lane - 18 * g;                     // lanes 54..63: g == 3, idle
    double2 sd{0.0, 0.0}, st{0.0, 0.0};
    for (int q = q0; q < q1; q += 3 * kGatherDepth) {
        int e[kGatherDepth];
#pragma unroll
        for (int u = 0; u < kGatherDepth; ++u) e[u] = list[min(q + 3 * u + g, q1 - 1)];
        double2 v[kGatherDepth];
        bool tr[kGatherDepth];
#pragma unroll
        for (int u = 0; u < kGatherDepth; ++u) {
            const int row = e[u] / (K * K), pr = e[u] - row * (K * K);
            const int sa = pr / K, sb = pr - sa * K;
            tr[u] = sa > sb;
            const double2 *src = reinterpret_cast<const double2 *>(partial + (size_t)row * NE + 36 * (tr[u] ? gn_sub(K, sb, sa) : gn_sub(K, sa, sb))) + h;
            v[u] = (g < 3 && q + 3 * u + g < q1) ? *src : double2{0.0, 0.0};
        }
#pragma unroll
        for (int u = 0; u < kGatherDepth; ++u) {
            sd.x += tr[u] ? 0.0 : v[u].x; sd.y += tr[u] ? 0.0 : v[u].y;
            st.x += tr[u] ? v[u].x : 0.0; st.y += tr[u] ? v[u].y : 0.0;
        }
    }
    if (g < 3) {
        comb[g][0][2 * h] = sd.x; comb[g][0][2 * h + 1] = sd.y;
        comb[g][1][2 * h] = st.x; comb[g][1][2 * h + 1] = st.y;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    double tot = 0.0;
    if (lane < 36) {
        const int m = lane, mt = 6 * (lane % 6) + lane / 6;
        tot = ((comb[0][0][m] + comb[1][0][m]) + comb[2][0][m]) + ((comb[0][1][mt] + comb[1][1][mt]) + comb[2][1][mt]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();                               // (the scratch is reused by the wave's next call)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    return tot;
}

// one workgroup = four blocks, one wave each; every wave of the workgroup must call this (it synchronises)
template <int K>
__device__ __forceinline__ double gather_block_both(const double *__restrict__ partial, const double *__restrict__ live,
                                                    const int *__restrict__ blk_ptr,
                                                    const int *__restrict__ blk_ent, const double *__restrict__ rpartial,
                                                    const int *__restrict__ rblk_ptr, const int *__restrict__ rblk_ent, int b, bool real,
                                                    int lane, int wv, GatherLds &L) {
    constexpr int NE = gn_row_stride(K), kLive = gn_row_entries(K);
    constexpr int NE2 = gn_row_stride(2), kLive2 = gn_row_entries(2);
    const int ia = (lane % 36) / 6, ib = lane % 6;
    double acc = 0.0, racc = 0.0;
    int nl = 0;
    bool coop = false;
    if (real) {
        // hop 1
        GT_STAMP(0);
        const int beg = blk_ptr[b], end = blk_ptr[b + 1];
        const int rbeg = rpartial ? rblk_ptr[b] : 0, rend = rpartial ? rblk_ptr[b + 1] : 0;
        GT_STAMP(1);
        if (end - beg > 256 || rend - rbeg > 64) {
            acc = gather_block_list<K>(partial, live, blk_ptr, blk_ent, b, lane, wv);
            if (rpartial) racc = gather_block_list<2>(rpartial, nullptr, rblk_ptr, rblk_ent, b, lane, wv);
        } else {
            // hop 2: entries
            int ent[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) ent[u] = beg + 64 * u + lane < end ? blk_ent[beg + 64 * u + lane] : -1;
            const int rent = rbeg + lane < rend ? rblk_ent[rbeg + lane] : -1;
            GT_STAMP(2);
            // hop 3: live flags
            // (flags first, tests after: `ent >= 0 && flag != 0` in one expression makes every load wait for the one before)
            double flag[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) flag[u] = ent[u] >= 0 ? (live ? live[ent[u] / (K * K)] : partial[(size_t)(ent[u] / (K * K)) * NE + kLive]) : 0.0;
            const double rflag = rent >= 0 ? rpartial[(size_t)(rent / 4) * NE2 + kLive2] : 0.0;
            bool on[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) on[u] = flag[u] != 0.0;
            const bool ron = rflag != 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const unsigned long long m = __ballot(on[u]);
                if (on[u]) L.liveD[wv][nl + __popcll(m & ((1ull << lane) - 1ull))] = ent[u];
                nl += __popcll(m);
            }
            const unsigned long long rm = __ballot(ron);
            if (ron) L.liveR[wv][__popcll(rm & ((1ull << lane) - 1ull))] = rent;
            const int rnl = __popcll(rm);
            __builtin_amdgcn_wave_barrier();
            GT_STAMP(3);
            coop = nl > kCoopList;
            // hop 4: values of both lists in flight together (regulariser: usually 1-2 entries)
            if (rnl > 0) racc = gather_rounds<2>(rpartial, L.liveR[wv], 0, rnl, lane, L.comb[wv]);
            if (!coop && nl > 0) acc = gather_rounds<K>(partial, L.liveD[wv], 0, nl, lane, L.comb[wv]);
#ifdef DFH_GATHER_TRACE
            if (lane == 0 && b < 8192)
                g_gather_trace[b][5] = (unsigned long long)(end - beg) | ((unsigned long long)nl << 16) | ((unsigned long long)(rend - rbeg) << 32) | ((unsigned long long)rnl << 48);
#endif
        }
    }
    if (lane == 0) L.coop[wv] = coop ? nl : 0;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int n = L.coop[w];
        if (n > 0) {                                              // (workgroup-uniform)
            const int seg = (n + 3) / 4, q0 = wv * seg, q1 = min(n, q0 + seg);
            const double sum = q0 < q1 ? gather_rounds<K>(partial, L.liveD[w], q0, q1, lane, L.comb[wv]) : 0.0;
            if (lane < 36) L.part[w][wv][lane] = sum;
        }
    }
    __syncthreads();
    if (coop && lane < 36) acc = ((L.part[wv][0][lane] + L.part[wv][1][lane]) + L.part[wv][2][lane]) + L.part[wv][3][lane];
    GT_STAMP(4);
    return acc + racc;
}

// one wave: J^T r of node a from its list; the total for unknown i ends up in lanes 0..5
template <int K>
__device__ __forceinline__ double gather_node_list(const double *__restrict__ partial, const double *__restrict__ live,
                                                   const int *__restrict__ node_ptr,
                                                   const int *__restrict__ node_ent, int a, int lane, int wv) {
    constexpr int NUP = gn_row_gram(K), NE = gn_row_stride(K), kLive = gn_row_entries(K);
    double acc = 0.0;
    const int j = lane / 6, i = lane - 6 * j;                  // lanes 60..63 idle
    __shared__ int sLive[4][64];
    const int beg = node_ptr[a], end = node_ptr[a + 1];
    for (int base = beg; base < end; base += 64) {
        // 64 entries and their rows' live flags at once; the live ones, compacted in list order, are then taken
        // ten at a time (lane group j takes the j-th of each ten) -- one value hop per ten entries
        const int n = min(64, end - base);
        int mine = lane < n ? node_ent[base + lane] : -1;
        const double flag = mine >= 0 ? (live ? live[mine / K] : partial[(size_t)(mine / K) * NE + kLive]) : 0.0;
        if (flag == 0.0) mine = -1;
        const unsigned long long live = __ballot(mine >= 0);
        if (mine >= 0) sLive[wv][__popcll(live & ((1ull << lane) - 1ull))] = mine;
        __builtin_amdgcn_wave_barrier();
        const int nl = __popcll(live);
        if (j < 10) {
            for (int m0 = j; m0 < nl; m0 += 80) {               // eight loads in flight per lane (absent entries add 0.0)
                int e[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) e[u] = sLive[wv][min(m0 + 10 * u, nl - 1)];
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int row = e[u] / K, slot = e[u] - row * K;
                    const double *src = partial + (size_t)row * NE + NUP + slot * 6 + i;
                    v[u] = m0 + 10 * u < nl ? *src : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += v[u];
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    double tot = acc;
#pragma unroll
    for (int k = 1; k < 10; ++k) {
        const double o = __shfl(acc, lane + 6 * k, 64);
        tot += (lane + 6 * k < 60) ? o : 0.0;
    }
    return tot;
}

// one workgroup: fixed-order sum of n_cc {cost, count} pairs cc_stride doubles apart; valid in thread 0
__device__ __forceinline__ void gather_cost(const double *__restrict__ cc, int n_cc, int cc_stride, double (*red)[64], double &c0,
                                            double &c1) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double c = 0.0, n = 0.0;
    for (int r = (int)threadIdx.x; r < n_cc; r += 256) {
        c += cc[(size_t)r * cc_stride];
        n += cc[(size_t)r * cc_stride + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { c += __shfl_xor(c, o, 64); n += __shfl_xor(n, o, 64); }
    __syncthreads();                                   // `red` may still be read from a previous call
    if (lane == 0) { red[0][wv] = c; red[1][wv] = n; }
    __syncthreads();
    c0 = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    c1 = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
}

// the regulariser's lists for the same launch (partial == NULL: none)
struct RegLists {
    const double *partial;
    const int *blk_ptr, *blk_ent, *node_ptr, *node_ent;
    int n_rows;
};

template <int K>
__global__ __launch_bounds__(256) void gn_gather_kernel(const double *__restrict__ partial, const double *__restrict__ live, int n_rows,
                                                        const int *__restrict__ blk_ptr,
                                                        const int *__restrict__ blk_ent, int n_blocks,
                                                        const int *__restrict__ node_ptr, const int *__restrict__ node_ent,
                                                        int n_nodes, double *__restrict__ vals, double *__restrict__ rhs,
                                                        double *__restrict__ cost_count, const double *__restrict__ cc, int n_cc,
                                                        int cc_stride, bool accumulate, int only_part, const RegLists rl,
                                                        const int2 *__restrict__ upper = nullptr, int n_upper = 0) {
    // upper (optional): J^T J is symmetric and so is the way its blocks are summed -- block (b, a)'s list holds the rows of block
    // (a, b)'s with the slots swapped, walked in the same order -- so only the n_upper blocks with column >= row are walked
    // (upper[u] = {block, its mirror block or -1 on the diagonal}) and each wave stores its sums twice, the second time
    // transposed: half the block waves, half the gather's reads.
    // cc: n_cc {cost, count} pairs, cc_stride doubles apart (per tile for the data term, per pair row for the regulariser)
    // only_part (debug timing): 0 = all, 1 = blocks, 2 = J^T r, 3 = cost
    // accumulate: add to what is there (a gather of its own for the regulariser rows) instead of storing
    const int nrw = (n_nodes + 3) / 4;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ double red[4][64];
    const int n_walk = upper ? n_upper : n_blocks;
    const int nbw = (n_walk + 3) / 4;
    if (only_part) {
        const int part_of = (int)blockIdx.x < nbw ? 1 : ((int)blockIdx.x < nbw + nrw ? 2 : 3);
        if (part_of != only_part) return;
    }
    if ((int)blockIdx.x < nbw) {
        __shared__ GatherLds L;
        // a workgroup's four blocks are a quarter of the block range apart: neighbouring blocks are the same node's row
        // and have long lists together, which one workgroup would walk alone
        const int u = wv * nbw + (int)blockIdx.x;
        const bool real = u < n_walk;
        int b = u, mir = -1;
        if (upper && real) { const int2 um = upper[u]; b = um.x; mir = um.y; }
        const double acc = gather_block_both<K>(partial, live, blk_ptr, blk_ent, rl.partial, rl.blk_ptr, rl.blk_ent, b, real, lane, wv, L);
        if (real && lane < 36) {
            double *dst = vals + 36 * (size_t)b + lane;
            *dst = accumulate ? *dst + acc : acc;
            if (mir >= 0) {
                double *dm = vals + 36 * (size_t)mir + 6 * (lane % 6) + lane / 6;
                *dm = accumulate ? *dm + acc : acc;
            }
        }
    } else if ((int)blockIdx.x < nbw + nrw) {
        const int a = ((int)blockIdx.x - nbw) * 4 + wv;
        if (a >= n_nodes) return;
        double tot = gather_node_list<K>(partial, live, node_ptr, node_ent, a, lane, wv);
        if (rl.partial) tot = tot + gather_node_list<2>(rl.partial, nullptr, rl.node_ptr, rl.node_ent, a, lane, wv);
        if (lane < 6) rhs[6 * a + lane] = accumulate ? rhs[6 * a + lane] + tot : tot;
    } else {
        double c0, c1;
        gather_cost(cc, n_cc, cc_stride, red, c0, c1);
        if (rl.partial) {
            double r0, r1;
            gather_cost(rl.partial + gn_row_gram(2) + 12, rl.n_rows, gn_row_stride(2), red, r0, r1);
            c0 = c0 + r0; c1 = c1 + r1;
        }
        if (threadIdx.x == 0) {
            cost_count[0] = accumulate ? cost_count[0] + c0 : c0;
            cost_count[1] = accumulate ? cost_count[1] + c1 : c1;
        }
    }
}

// Regularisation rows rho_ij = c_ij (W(q_i,v_j) - W(q_j,v_j)): one WAVE per (i, slot); lanes 0..35
// own one entry (a,b) of the four 6x6 blocks (ii, jj, ij, ji), lanes 0..5 also the gradient, so the
// ~150 fp64 atomics of a pair are issued side by side instead of one after the other.
__device__ void gn_reg_pairs(int block, const int *__restrict__ node_nbr, int N, int k, const double *__restrict__ node_dq,
                             const double *__restrict__ node_pos, const double *__restrict__ node_w, double rw,
                             const int *__restrict__ row_ptr, const int *__restrict__ col, double *__restrict__ vals,
                             double *__restrict__ rhs, double *__restrict__ cost_count, double *__restrict__ partial_reg) {
    // partial_reg != NULL (planned build): the pair's {upper triangle of the 12x12 Gram matrix of [J_i | J_j] |
    // J^T rho | 0.5 rho^2 | 0} is STORED in row t (92 doubles) and gathered like a 2-node data row: no atomics.
    // rows of the K = 2 layout: sub-blocks (i,i) (i,j) (j,j) | J^T rho (12) | cost | count | live flag
    constexpr int NE2 = gn_row_stride(2), kLive2 = gn_row_entries(2), kJtr2 = gn_row_gram(2), kCost2 = gn_row_gram(2) + 12;
    const int t = block * (int)(blockDim.x >> 6) + (threadIdx.x >> 6);      // one wave per node pair
    const int lane = threadIdx.x & 63;
    if (t >= N * k) return;
    const int i = t / k;
    const int j = node_nbr[t];
    if (i == j) {                                                  // zero rows, zero Jacobian
        if (partial_reg && lane == 0) {                           // dead row (its cost / count are read unconditionally)
            partial_reg[(size_t)t * NE2 + kLive2] = 0.0;
            partial_reg[(size_t)t * NE2 + kCost2] = 0.0;
            partial_reg[(size_t)t * NE2 + kCost2 + 1] = 0.0;
        }
        return;
    }
    const double vx = round_f32(node_pos[3 * j]), vy = round_f32(node_pos[3 * j + 1]), vz = round_f32(node_pos[3 * j + 2]);
    const double *qi = node_dq + 8 * i, *qj = node_dq + 8 * j;
    const D3 yi = dqb_warp_exact(qi, vx, vy, vz);
    const D3 yj = dqb_warp_exact(qj, vx, vy, vz);
    const double wi = node_w[i], wj = node_w[j];
    const double c = rw * (wi > wj ? wi : wj);
    const double rho[3] = {c * (yi.x - yj.x), c * (yi.y - yj.y), c * (yi.z - yj.z)};
    const double si = (qi[0] * qi[0] + qi[1] * qi[1]) + (qi[2] * qi[2] + qi[3] * qi[3]);
    const double sj = (qj[0] * qj[0] + qj[1] * qj[1]) + (qj[2] * qj[2] + qj[3] * qj[3]);
    // J_i = c [ -[y_i]x | s_i I ],  J_j = -c [ -[y_j]x | s_j I ]   (3 x 6 each), column `col6` on demand
    auto Jcol = [&](const D3 &y, double sgn, double sc, int col6, double (&out)[3]) {
        // -[y]x = [[0, y2, -y1], [-y2, 0, y0], [y1, -y0, 0]]
        const double m[3][3] = {{0.0, y.z, -y.y}, {-y.z, 0.0, y.x}, {y.y, -y.x, 0.0}};
#pragma unroll
        for (int r = 0; r < 3; ++r) out[r] = col6 < 3 ? sgn * c * m[r][col6 % 3] : (r == col6 - 3 ? sgn * c * sc : 0.0);
    };
    if (lane < 36) {
        const int a = lane / 6, b = lane - 6 * a;
        double ia[3], ib[3], ja[3], jb[3];
        Jcol(yi, 1.0, si, a, ia); Jcol(yi, 1.0, si, b, ib);
        Jcol(yj, -1.0, sj, a, ja); Jcol(yj, -1.0, sj, b, jb);
        const double vii = (ia[0] * ib[0] + ia[1] * ib[1]) + ia[2] * ib[2];
        const double vjj = (ja[0] * jb[0] + ja[1] * jb[1]) + ja[2] * jb[2];
        const double vij = (ia[0] * jb[0] + ia[1] * jb[1]) + ia[2] * jb[2];
        const double vji = (ja[0] * ib[0] + ja[1] * ib[1]) + ja[2] * ib[2];
        if (partial_reg) {
            double *P = partial_reg + (size_t)t * NE2;
            P[gn_gram_index(2, 0, 0, a, b)] = vii;                 // (whole 6x6 sub-blocks: lane (b,a) computes the same products)
            P[gn_gram_index(2, 1, 1, a, b)] = vjj;
            P[gn_gram_index(2, 0, 1, a, b)] = vij;
            if (lane < 6) {
                double gi[3], gj[3];
                Jcol(yi, 1.0, si, lane, gi); Jcol(yj, -1.0, sj, lane, gj);
                P[kJtr2 + lane] = (gi[0] * rho[0] + gi[1] * rho[1]) + gi[2] * rho[2];
                P[kJtr2 + 6 + lane] = (gj[0] * rho[0] + gj[1] * rho[1]) + gj[2] * rho[2];
            }
            if (lane == 0) { P[kCost2] = 0.5 * ((rho[0] * rho[0] + rho[1] * rho[1]) + rho[2] * rho[2]); P[kCost2 + 1] = 0.0; P[kLive2] = 1.0; }
            return;
        }
        const int bii = find_block(row_ptr, col, i, i), bjj = find_block(row_ptr, col, j, j);
        const int bij = find_block(row_ptr, col, i, j), bji = find_block(row_ptr, col, j, i);
        if (bii >= 0 && vii != 0.0) atomicAdd(vals + 36 * (size_t)bii + lane, vii);
        if (bjj >= 0 && vjj != 0.0) atomicAdd(vals + 36 * (size_t)bjj + lane, vjj);
        if (bij >= 0 && vij != 0.0) atomicAdd(vals + 36 * (size_t)bij + lane, vij);
        if (bji >= 0 && vji != 0.0) atomicAdd(vals + 36 * (size_t)bji + lane, vji);
        if (lane < 6) {
            double gi[3], gj[3];
            Jcol(yi, 1.0, si, lane, gi); Jcol(yj, -1.0, sj, lane, gj);
            atomicAdd(rhs + 6 * i + lane, (gi[0] * rho[0] + gi[1] * rho[1]) + gi[2] * rho[2]);
            atomicAdd(rhs + 6 * j + lane, (gj[0] * rho[0] + gj[1] * rho[1]) + gj[2] * rho[2]);
        }
        if (lane == 0) atomicAdd(cost_count, 0.5 * ((rho[0] * rho[0] + rho[1] * rho[1]) + rho[2] * rho[2]));
    }
}

__global__ __launch_bounds__(256) void gn_build_reg_kernel(const int *__restrict__ node_nbr, int N, int k,
                                                            const double *__restrict__ node_dq,
                                                            const double *__restrict__ node_pos,
                                                            const double *__restrict__ node_w, double rw,
                                                            const int *__restrict__ row_ptr, const int *__restrict__ col,
                                                            double *__restrict__ vals, double *__restrict__ rhs,
                                                            double *__restrict__ cost_count, double *__restrict__ partial_reg) {
    gn_reg_pairs((int)blockIdx.x, node_nbr, N, k, node_dq, node_pos, node_w, rw, row_ptr, col, vals, rhs, cost_count, partial_reg);
}

// gn_gather_kernel<knn> for a term built outside this file (the landmark rows, dfh_landmarks.hip): the instantiations above, no
// regulariser lists, every part of the gather.
int gn_gather_launch(int knn, const double *partial, const double *live, int n_rows, const int *blk_ptr, const int *blk_ent, int n_blocks,
                     const int *node_ptr, const int *node_ent, int n_nodes, double *vals, double *rhs, double *cost_count, const double *cc,
                     int n_cc, bool accumulate, const int *upper, int n_upper, void *stream) {
    const int2 *up = (upper && n_upper > 0) ? reinterpret_cast<const int2 *>(upper) : nullptr;
    const int n_walk = up ? n_upper : n_blocks;
    dim3 grid((unsigned)((n_walk + 3) / 4 + (n_nodes + 3) / 4 + 1)), block(256);
#define DFH_GATHER_TERM(KK)                                                                                         \
    case KK:                                                                                                        \
        hipLaunchKernelGGL(gn_gather_kernel<KK>, grid, block, 0, (hipStream_t)stream, partial, live, n_rows, blk_ptr, blk_ent, n_blocks, \
                           node_ptr, node_ent, n_nodes, vals, rhs, cost_count, cc, n_cc, 2, accumulate, 0, RegLists{}, up, n_upper);    \
        break
    switch (knn) {
        DFH_GATHER_TERM(1); DFH_GATHER_TERM(2); DFH_GATHER_TERM(3); DFH_GATHER_TERM(4);
        DFH_GATHER_TERM(5); DFH_GATHER_TERM(6); DFH_GATHER_TERM(7); DFH_GATHER_TERM(8);
    }
#undef DFH_GATHER_TERM
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

}  // namespace dfh

// =================================================================================== C ABI
extern "C" {

int dfh_gn_associate(const dfh_gn_problem *problem, const dfh_gn_frame *frame, void *stream) {
    using namespace dfh;
    int rc = check_problem("dfh_gn_associate", problem, false);
    if (rc == DFH_OK) rc = check_frame("dfh_gn_associate", frame, false);
    if (rc != DFH_OK) return rc;
    const dfh_gn_problem &q = *problem;
    if (q.n_samples == 0) return DFH_OK;
    const AssocArgs aa = assoc_args(q, *frame, false);
    dim3 grid((q.n_samples + 255) / 256), block(256);
    if (frame->depth_dtype == DFH_F32) {
        hipLaunchKernelGGL(associate_kernel<float>, grid, block, 0, (hipStream_t)stream, q.sample_pos, q.nbr, q.weights, q.n_samples,
                           q.node_dq, aa.ap, q.corr, q.valid, aa.views, aa.n_views);
    } else {
        hipLaunchKernelGGL(associate_kernel<double>, grid, block, 0, (hipStream_t)stream, q.sample_pos, q.nbr, q.weights, q.n_samples,
                           q.node_dq, aa.ap, q.corr, q.valid, aa.views, aa.n_views);
    }
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_gn_associate_gated(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_normal_gate *gate, void *stream) {
    using namespace dfh;
    const char *what = "dfh_gn_associate_gated";
    int rc = check_problem(what, problem, false);
    if (rc == DFH_OK) rc = check_frame(what, frame, false);
    if (rc == DFH_OK) rc = check_gate(what, gate);
    if (rc != DFH_OK) return rc;
    const dfh_gn_problem &q = *problem;
    if (q.n_samples == 0) return DFH_OK;
    const GatedAssocArgs ga = gated_assoc_args(q, *frame, *gate, false);
    dim3 grid((q.n_samples + 255) / 256), block(256);
    if (frame->depth_dtype == DFH_F32) {
        hipLaunchKernelGGL(associate_gated_kernel<float>, grid, block, 0, (hipStream_t)stream, q.sample_pos, q.sample_nrm, q.nbr, q.weights,
                           q.n_samples, q.node_dq, ga.ap, q.corr, q.valid, ga.views, ga.n_views, ga.ng);
    } else {
        hipLaunchKernelGGL(associate_gated_kernel<double>, grid, block, 0, (hipStream_t)stream, q.sample_pos, q.sample_nrm, q.nbr, q.weights,
                           q.n_samples, q.node_dq, ga.ap, q.corr, q.valid, ga.views, ga.n_views, ga.ng);
    }
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

// The table travels as kernel arguments of a one-workgroup launch that writes it to device memory (a hipMemcpyAsync from
// pageable host memory is staged by the runtime and stalls the stream for tens of microseconds)
namespace dfh {
constexpr int kViewChunk = 16;
struct ViewChunk { AssocView v[kViewChunk]; };
static_assert(sizeof(ViewChunk) + 16 <= 4096, "the chunk must fit the kernel-argument segment");
__global__ __launch_bounds__(256) void upload_views_kernel(AssocView *dst, const ViewChunk c, int n) {
    typedef const unsigned long long __attribute__((address_space(4))) *KernArgWords;
    KernArgWords ka = (KernArgWords)__builtin_amdgcn_kernarg_segment_ptr() + 1;                                          // behind `dst`
    unsigned long long *out = reinterpret_cast<unsigned long long *>(dst);
    const int words = n * (int)(sizeof(AssocView) / 8);
    for (int i = threadIdx.x; i < words; i += 256) out[i] = ka[i];
    (void)c;
}
}  // namespace dfh

namespace dfh {
// {smallest, largest} valid z = -depth of every 16 x 16-pixel cell of every view (no valid pixel: {inf, 0}); block = cell
__global__ __launch_bounds__(256) void view_cells_kernel(const AssocView *__restrict__ views, int H, int W) {
    __shared__ float smin[4], smax[4];
    const AssocView &vw = views[blockIdx.y];
    const int ncx = (W + kCellPx - 1) / kCellPx;
    const int cy = blockIdx.x / ncx, cx = blockIdx.x - cy * ncx;
    const int x = cx * kCellPx + (threadIdx.x & 15), y = cy * kCellPx + (threadIdx.x >> 4);
    float z = 0.0f;
    if (x < W && y < H) z = -static_cast<const float *>(vw.depth)[(size_t)y * W + x];
    float lo = z > 0.0f ? z : __builtin_huge_valf(), hi = z > 0.0f ? z : 0.0f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float *out = const_cast<float *>(vw.cells) + 2 * (size_t)blockIdx.x;
        out[0] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
        out[1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    }
}
}  // namespace dfh

static size_t views_cells_offset(int n_views) { return ((size_t)n_views * sizeof(dfh::AssocView) + 255) & ~(size_t)255; }
static size_t view_cells_floats(int H, int W) {
    return 2 * (size_t)((W + dfh::kCellPx - 1) / dfh::kCellPx) * (size_t)((H + dfh::kCellPx - 1) / dfh::kCellPx);
}

size_t dfh_gn_views_bytes(int n_views, int depth_dtype, int H, int W) {
    if (n_views <= 0 || H <= 0 || W <= 0) return 0;
    if (depth_dtype == DFH_F64) return (size_t)n_views * sizeof(dfh::AssocView);
    if (depth_dtype != DFH_F32) return 0;
    return views_cells_offset(n_views) + (size_t)n_views * view_cells_floats(H, W) * sizeof(float);
}

// the inverse of an extrinsic's 3x3 part (adjugate)
static int invert_rotation(const double m[12], double Rinv[9]) {
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    DFH_REQUIRE(det != 0.0, "dfh_gn_pack_views: singular extrinsic");
    const double id = 1.0 / det;
    Rinv[0] = (e * i - f * h) * id; Rinv[1] = (c * h - b * i) * id; Rinv[2] = (b * f - c * e) * id;
    Rinv[3] = (f * g - d * i) * id; Rinv[4] = (a * i - c * g) * id; Rinv[5] = (c * d - a * f) * id;
    Rinv[6] = (d * h - e * g) * id; Rinv[7] = (b * g - a * h) * id; Rinv[8] = (a * e - b * d) * id;
    return DFH_OK;
}

int dfh_gn_pack_views(void *out, int n_views, const void *const *depth, int depth_dtype, int H, int W, const double *lw_cam,
                      void *stream) {
    using namespace dfh;
    DFH_REQUIRE(out && depth && lw_cam, "dfh_gn_pack_views: null pointer");
    DFH_REQUIRE(n_views >= 1 && n_views <= DFH_GN_MAX_VIEWS, "dfh_gn_pack_views: %d views (1..%d)", n_views, DFH_GN_MAX_VIEWS);
    DFH_REQUIRE(depth_dtype == DFH_F32 || depth_dtype == DFH_F64, "dfh_gn_pack_views: bad depth_dtype");
    DFH_REQUIRE(H >= 2 && W >= 2, "dfh_gn_pack_views: bad depth map size");
    static_assert(DFH_GN_MAX_VIEWS <= kViewChunk, "one upload launch");
    const bool cells = depth_dtype == DFH_F32;
    ViewChunk c;
    std::memset(&c, 0, sizeof c);
    for (int v = 0; v < n_views; ++v) {
        DFH_REQUIRE(depth[v], "dfh_gn_pack_views: depth map %d is null", v);
        const double *m = lw_cam + 12 * v;
        const int rc = invert_rotation(m, c.v[v].Rinv);
        if (rc != DFH_OK) return rc;
        for (int i = 0; i < 12; ++i) c.v[v].lw_cam[i] = m[i];
        c.v[v].depth = depth[v];
        if (cells) {
            c.v[v].cells = reinterpret_cast<const float *>(static_cast<char *>(out) + views_cells_offset(n_views)) + (size_t)v * view_cells_floats(H, W);
            // the depth-interval test of tile_view_mask needs |R x| = |x|: R^T R = I to 1e-9 (what a camera pose is)
            double worst = 0.0;
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    const double g = m[a] * m[b] + m[4 + a] * m[4 + b] + m[8 + a] * m[8 + b];
                    worst = std::fmax(worst, std::fabs(g - (a == b ? 1.0 : 0.0)));
                }
            c.v[v].cull_ok = worst <= 1e-9 ? 1.0 : 0.0;
        }
    }
    hipLaunchKernelGGL(upload_views_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, static_cast<AssocView *>(out), c, n_views);
    if (cells) {
        const unsigned ncell = (unsigned)(view_cells_floats(H, W) / 2);
        hipLaunchKernelGGL(view_cells_kernel, dim3(ncell, (unsigned)n_views), dim3(256), 0, (hipStream_t)stream,
                           static_cast<const AssocView *>(out), H, W);
    }
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

// The association fused into the data-row kernel (the caller checked that there is a plan): against the frame's views, against
// a live volume, against the views through the normal gate, or (all null) none.
struct BuildAssoc {
    const dfh::AssocArgs *views;
    const dfh::VolAssocArgs *vol;
    const dfh::GatedAssocArgs *gated = nullptr;
};

// zero_ptr / zero_count: doubles the launch's last workgroups clear (*zeroed says whether they did).  The problem is checked
// by the caller.
static int gn_build_impl(const dfh_gn_problem &q, const BuildAssoc &ba, void *stream, double *zero_ptr = nullptr,
                         size_t zero_count = 0, bool *zeroed = nullptr) {
    using namespace dfh;
    const AssocArgs *assoc = ba.views;
    if (zeroed) *zeroed = false;
    const int knn = q.knn, n_samples = q.n_samples, n_nodes = q.n_nodes, n_blocks = q.n_blocks, n_rows = q.n_rows;
    double *vals = q.vals, *rhs = q.rhs, *cost_count = q.cost_count, *partial = q.partial, *partial_reg = q.partial_reg;
    const bool planned = q.blk_ptr != nullptr;
    const bool planned_reg = planned && partial_reg != nullptr;
    hipStream_t s = (hipStream_t)stream;
    const int n_tiles = (n_samples + kTile - 1) / kTile;
    // planned build: the regulariser's pair rows ride along in the data-row launch (they only write partial_reg)
    const bool reg_in_data_launch = planned_reg && q.node_nbr && q.rw != 0.0 && n_samples > 0 && !on(opt().gn_reg_own_launch);
    double *tile_cost = planned && partial ? partial + (size_t)n_rows * gn_row_stride(knn) : nullptr;   // 2 doubles per tile, behind the rows; then one live flag per row
    if (planned) {
        // every block / rhs entry / cost is written by the gather, and every row of `partial` by the tile pass (rows
        // without a valid sample this iteration are zeroed there): nothing to clear
    } else if (rhs == vals + 36 * (size_t)n_blocks && cost_count == rhs + 6 * (size_t)n_nodes) {
        // the flat {blocks | rhs | cost,count} layout of the host solver: one memset
        DFH_HIP_CHECK(hipMemsetAsync(vals, 0, sizeof(double) * (36 * (size_t)n_blocks + 6 * (size_t)n_nodes + 2), s));
    } else {
        DFH_HIP_CHECK(hipMemsetAsync(vals, 0, sizeof(double) * 36 * (size_t)n_blocks, s));
        DFH_HIP_CHECK(hipMemsetAsync(rhs, 0, sizeof(double) * 6 * (size_t)n_nodes, s));
        DFH_HIP_CHECK(hipMemsetAsync(cost_count, 0, sizeof(double) * 2, s));
    }
    if (n_samples > 0) {
        BuildParams p;
        for (int i = 0; i < 8; ++i) p.lw.q[i] = q.lw_dq[i];
        p.S = n_samples; p.k = knn; p.N = n_nodes; p.huber = q.huber_delta;
        RegTail rt = {};
        rt.n_tiles = n_tiles;
        if (reg_in_data_launch) {
            rt.node_nbr = q.node_nbr; rt.node_pos = q.node_pos; rt.node_w = q.node_w; rt.partial_reg = partial_reg;
            rt.rw = q.rw; rt.N = n_nodes; rt.k = knn;
        }
        unsigned n_wg = (unsigned)(n_tiles + (reg_in_data_launch ? (n_nodes * knn + kTileWaves - 1) / kTileWaves : 0));
        if (planned && zero_ptr && zero_count > 0 && (zero_count + kZeroPerWg - 1) / kZeroPerWg < (1u << 20)) {
            rt.zero_ptr = zero_ptr; rt.zero_count = zero_count; rt.first_zero_wg = (int)n_wg;
            n_wg += (unsigned)((zero_count + kZeroPerWg - 1) / kZeroPerWg);
            if (zeroed) *zeroed = true;
        }
        dim3 grid(n_wg), block(kTile);
        const AssocArgs aa = assoc ? *assoc : AssocArgs{};
#define DFH_BUILD(KK)                                                                                               \
    case KK:                                                                                                        \
        if (ba.vol)                                                                                                 \
            hipLaunchKernelGGL((gn_build_data_kernel<KK, true, AssocMode::Volume>), grid, block, 0, s, q.sample_pos, q.sample_nrm, q.nbr, q.weights, \
                               q.corr, q.valid, q.node_dq, p, q.row_ptr, q.col, vals, rhs, cost_count, q.run_id, partial, tile_cost, rt, *ba.vol); \
        else if (ba.gated)                                                                                          \
            hipLaunchKernelGGL((gn_build_data_kernel<KK, true, AssocMode::ViewsGated>), grid, block, 0, s, q.sample_pos, q.sample_nrm, q.nbr, q.weights, \
                               q.corr, q.valid, q.node_dq, p, q.row_ptr, q.col, vals, rhs, cost_count, q.run_id, partial, tile_cost, rt, *ba.gated); \
        else if (assoc)                                                                                             \
            hipLaunchKernelGGL((gn_build_data_kernel<KK, true, AssocMode::Views>), grid, block, 0, s, q.sample_pos, q.sample_nrm, q.nbr, q.weights, \
                               q.corr, q.valid, q.node_dq, p, q.row_ptr, q.col, vals, rhs, cost_count, q.run_id, partial, tile_cost, rt, aa); \
        else if (planned)                                                                                           \
            hipLaunchKernelGGL((gn_build_data_kernel<KK, true, AssocMode::None>), grid, block, 0, s, q.sample_pos, q.sample_nrm, q.nbr, q.weights, \
                               q.corr, q.valid, q.node_dq, p, q.row_ptr, q.col, vals, rhs, cost_count, q.run_id, partial, tile_cost, rt, aa); \
        else                                                                                                        \
            hipLaunchKernelGGL((gn_build_data_kernel<KK, false, AssocMode::None>), grid, block, 0, s, q.sample_pos, q.sample_nrm, q.nbr, q.weights, \
                               q.corr, q.valid, q.node_dq, p, q.row_ptr, q.col, vals, rhs, cost_count, q.run_id, partial, tile_cost, rt, aa); \
        break
        switch (knn) {
            DFH_BUILD(1); DFH_BUILD(2); DFH_BUILD(3); DFH_BUILD(4); DFH_BUILD(5); DFH_BUILD(6); DFH_BUILD(7); DFH_BUILD(8);
        }
#undef DFH_BUILD
        DFH_HIP_CHECK(hipGetLastError());
    }
    const int dbg_part = opt().dbg_gather_part > 0 ? (int)opt().dbg_gather_part : 0;
    // the regulariser's lists ride along in the data rows' gather when its rows were built in the data-row launch
    RegLists rl = {};
    const bool reg_in_gather = reg_in_data_launch && !on(opt().gn_reg_own_gather);
    if (reg_in_gather) {
        rl.partial = partial_reg; rl.blk_ptr = q.rblk_ptr; rl.blk_ent = q.rblk_ent; rl.node_ptr = q.rnode_ptr; rl.node_ent = q.rnode_ent;
        rl.n_rows = n_nodes * knn;
    }
    if (planned) {
        const int n_upper = q.n_upper;
        const int2 *upper = (q.blk_upper && n_upper > 0 && !on(opt().gn_gather_full)) ? reinterpret_cast<const int2 *>(q.blk_upper) : nullptr;
        const int n_walk = upper ? n_upper : n_blocks;
        dim3 grid((unsigned)((n_walk + 3) / 4 + (n_nodes + 3) / 4 + 1)), block(256);
#define DFH_GATHER(KK)                                                                                              \
    case KK:                                                                                                        \
        hipLaunchKernelGGL(gn_gather_kernel<KK>, grid, block, 0, s, partial, tile_cost + 2 * (size_t)n_tiles, n_rows, q.blk_ptr, q.blk_ent, n_blocks, \
                           q.node_ptr, q.node_ent, n_nodes, vals, rhs, cost_count, tile_cost, n_tiles, 2, false, dbg_part, rl, upper, n_upper);  \
        break
        switch (knn) {
            DFH_GATHER(1); DFH_GATHER(2); DFH_GATHER(3); DFH_GATHER(4); DFH_GATHER(5); DFH_GATHER(6); DFH_GATHER(7); DFH_GATHER(8);
        }
#undef DFH_GATHER
        DFH_HIP_CHECK(hipGetLastError());
    }
    if (q.node_nbr && q.rw != 0.0) {
        const int n = n_nodes * knn;
        if (!reg_in_data_launch)
            hipLaunchKernelGGL(gn_build_reg_kernel, dim3((n + 3) / 4), dim3(256), 0, s, q.node_nbr, n_nodes, knn, q.node_dq, q.node_pos,
                               q.node_w, q.rw, q.row_ptr, q.col, vals, rhs, cost_count, planned_reg ? partial_reg : nullptr);
        if (planned_reg && !reg_in_gather) {
            dim3 grid((unsigned)((n_blocks + 3) / 4 + (n_nodes + 3) / 4 + 1)), block(256);
            hipLaunchKernelGGL(gn_gather_kernel<2>, grid, block, 0, s, partial_reg, (const double *)nullptr, n, q.rblk_ptr, q.rblk_ent, n_blocks,
                               q.rnode_ptr, q.rnode_ent, n_nodes, vals, rhs, cost_count, partial_reg + gn_row_gram(2) + 12, n, gn_row_stride(2),
                               true, dbg_part, RegLists{});
        }
        DFH_HIP_CHECK(hipGetLastError());
    }
    return DFH_OK;
}

int dfh_gn_build(const dfh_gn_problem *problem, const dfh_gn_frame *frame, void *stream) {
    using namespace dfh;
    int rc = check_problem("dfh_gn_build", problem, true);
    if (rc == DFH_OK && frame) rc = check_frame("dfh_gn_build", frame, true);
    if (rc != DFH_OK) return rc;
    if (!frame) return gn_build_impl(*problem, BuildAssoc{nullptr, nullptr}, stream);
    DFH_REQUIRE(problem->blk_ptr, "dfh_gn_build: association inside the build needs a plan");
    const AssocArgs aa = assoc_args(*problem, *frame, true);
    return gn_build_impl(*problem, BuildAssoc{&aa, nullptr}, stream);
}

// the checks the fused gated entry points share; *ga <- the data-row kernel's arguments
static int check_fused_gated(const char *what, const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_normal_gate *gate,
                             dfh::GatedAssocArgs *ga) {
    using namespace dfh;
    int rc = check_problem(what, problem, true);
    if (rc == DFH_OK) rc = check_frame(what, frame, true);
    if (rc == DFH_OK) rc = check_gate(what, gate);
    if (rc != DFH_OK) return rc;
    DFH_REQUIRE(problem->blk_ptr, "%s: null blk_ptr (the fused association needs a plan)", what);
    *ga = gated_assoc_args(*problem, *frame, *gate, true);
    return DFH_OK;
}

int dfh_gn_build_gated(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_normal_gate *gate, void *stream) {
    dfh::GatedAssocArgs ga;
    const int rc = check_fused_gated("dfh_gn_build_gated", problem, frame, gate, &ga);
    if (rc != DFH_OK) return rc;
    if (problem->n_samples == 0) return DFH_OK;                      // (nothing to gate: dfh_gn_build builds the sample-less system)
    return gn_build_impl(*problem, BuildAssoc{nullptr, nullptr, &ga}, stream);
}

// the checks the fused volume entry points share; *va <- the data-row kernel's arguments
static int check_fused_volume(const char *what, const dfh_gn_problem *problem, const dfh_gn_volume_term *term, dfh::VolAssocArgs *va) {
    using namespace dfh;
    int rc = check_problem(what, problem, true);
    if (rc == DFH_OK) rc = check_volume_term(what, term, true);
    if (rc != DFH_OK) return rc;
    DFH_REQUIRE(problem->blk_ptr, "%s: null blk_ptr (the fused association needs a plan)", what);
    *va = vol_assoc_args(*problem, *term);
    return DFH_OK;
}

int dfh_gn_build_volume(const dfh_gn_problem *problem, const dfh_gn_volume_term *term, void *stream) {
    dfh::VolAssocArgs va;
    const int rc = check_fused_volume("dfh_gn_build_volume", problem, term, &va);
    if (rc != DFH_OK) return rc;
    return gn_build_impl(*problem, BuildAssoc{nullptr, &va}, stream);
}

size_t dfh_gn_partial_doubles(int knn) {
    if (knn < 1 || knn > dfh::kKMaxS) return 0;
    return (size_t)dfh::gn_row_stride(knn);
}

#ifdef DFH_BUILD_TRACE
int dfh_debug_build_trace(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(dfh::g_build_trace), sizeof(unsigned long long) * 8192 * 8) == hipSuccess ? 0 : -1;
}
#endif

#ifdef DFH_GATHER_TRACE
int dfh_debug_gather_trace(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(dfh::g_gather_trace), sizeof(unsigned long long) * 8192 * 8) == hipSuccess ? 0 : -1;
}
#endif

// The body of dfh_gn_solve / dfh_gn_solve_volume: the problem, its plan and the association's arguments are checked by the caller.
// lm (optional): a checked landmark term, added to the system after every build (dfh_gn_solve_landmarks); NULL: none.
// ph (optional): a checked photometric term with its frame pf, added after the landmark term (dfh_gn_solve_photometric); NULL: none.
static int gn_solve_impl(const char *what, const dfh_gn_problem &q, const BuildAssoc &ba, const dfh_gn_solve_params *params, void *stream,
                         const dfh_gn_landmarks *lm = nullptr, const dfh_gn_photometric *ph = nullptr, const dfh_gn_frame *pf = nullptr) {
    using namespace dfh;
    DFH_REQUIRE(params, "%s: null params", what);
    const dfh_gn_solve_params &sp = *params;
    DFH_REQUIRE(sp.n_iters >= 0 && sp.n_iters <= 1000, "%s: %d iterations", what, sp.n_iters);
    DFH_REQUIRE(sp.n_global >= 0 && sp.n_global <= 100, "%s: %d rigid-mode steps", what, sp.n_global);
    DFH_REQUIRE(sp.pcg_iters >= 1 && sp.x_out && sp.pcg_workspace, "%s: bad solve arguments", what);
    DFH_REQUIRE(sp.pcg_workspace_bytes >= dfh_pcg_workspace_bytes(q.n_nodes, sp.pcg_iters), "%s: solve workspace too small", what);
    if (ba.gated && q.n_samples == 0) return DFH_OK;                 // (nothing to gate: dfh_gn_solve runs the sample-less schedule)
    int rc;
    for (int g = 0; g < sp.n_global; ++g) {
        rc = gn_build_impl(q, ba, stream);
        if (rc == DFH_OK && lm) rc = gn_add_landmarks_impl(q, *lm, stream);
        if (rc == DFH_OK && ph) rc = gn_add_photometric_impl(q, *pf, *ph, stream);
        if (rc != DFH_OK) return rc;
        rc = dfh_gn_global_step(q.vals, q.n_blocks, q.rhs, q.n_nodes, sp.global_lm, q.node_dq, sp.global_xi_out, sp.global_scratch,
                                sp.global_scratch_bytes, stream);
        if (rc != DFH_OK) return rc;
    }
    // the frame's iterations are queued back to back from here: nothing between them depends on the host
    double *zbegin = nullptr;
    size_t zcount = 0;
    pcg_zero_range(sp.pcg_workspace, q.n_nodes, sp.pcg_iters, &zbegin, &zcount);
    for (int it = 0; it < sp.n_iters; ++it) {
        bool zeroed = false;
        rc = gn_build_impl(q, ba, stream, on(opt().gn_iter_own_clear) ? nullptr : zbegin, zcount, &zeroed);
        if (rc == DFH_OK && lm) rc = gn_add_landmarks_impl(q, *lm, stream);
        if (rc == DFH_OK && ph) rc = gn_add_photometric_impl(q, *pf, *ph, stream);
        if (rc != DFH_OK) return rc;
        rc = pcg_solve_impl(q.row_ptr, q.col, q.vals, q.rhs, q.n_nodes, sp.pcg_iters, sp.lm_abs, sp.lm_rel, sp.x_out, sp.pcg_workspace,
                            sp.pcg_workspace_bytes, q.node_dq, sp.step, stream, zeroed);
        if (rc != DFH_OK) return rc;
    }
    return DFH_OK;
}

int dfh_gn_solve(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_solve_params *params, void *stream) {
    using namespace dfh;
    int rc = check_problem("dfh_gn_solve", problem, true);
    if (rc == DFH_OK) rc = check_frame("dfh_gn_solve", frame, true);
    if (rc != DFH_OK) return rc;
    DFH_REQUIRE(problem->blk_ptr, "dfh_gn_solve: null blk_ptr (the fused association needs a plan)");
    const AssocArgs aa = assoc_args(*problem, *frame, true);
    return gn_solve_impl("dfh_gn_solve", *problem, BuildAssoc{&aa, nullptr}, params, stream);
}

int dfh_gn_solve_landmarks(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_landmarks *landmarks,
                           const dfh_gn_solve_params *params, void *stream) {
    using namespace dfh;
    const char *what = "dfh_gn_solve_landmarks";
    int rc = check_problem(what, problem, true);
    if (rc == DFH_OK && frame) rc = check_frame(what, frame, true);
    if (rc == DFH_OK) rc = check_landmarks(what, landmarks);
    if (rc != DFH_OK) return rc;
    DFH_REQUIRE(problem->blk_ptr, "dfh_gn_solve_landmarks: null blk_ptr (the solve needs a plan)");
    if (!frame) return gn_solve_impl(what, *problem, BuildAssoc{nullptr, nullptr}, params, stream, landmarks);
    const AssocArgs aa = assoc_args(*problem, *frame, true);
    return gn_solve_impl(what, *problem, BuildAssoc{&aa, nullptr}, params, stream, landmarks);
}

int dfh_gn_solve_photometric(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_landmarks *landmarks,
                             const dfh_gn_photometric *photo, const dfh_gn_solve_params *params, void *stream) {
    using namespace dfh;
    if (!photo) return landmarks ? dfh_gn_solve_landmarks(problem, frame, landmarks, params, stream) : dfh_gn_solve(problem, frame, params, stream);
    const char *what = "dfh_gn_solve_photometric";
    int rc = check_problem(what, problem, true);
    if (rc == DFH_OK) rc = check_photometric(what, photo, frame, true);
    if (rc == DFH_OK && landmarks) rc = check_landmarks(what, landmarks);
    if (rc != DFH_OK) return rc;
    DFH_REQUIRE(problem->blk_ptr, "dfh_gn_solve_photometric: null blk_ptr (the solve needs a plan)");
    const AssocArgs aa = assoc_args(*problem, *frame, true);
    return gn_solve_impl(what, *problem, BuildAssoc{&aa, nullptr}, params, stream, landmarks, photo, frame);
}

int dfh_gn_solve_gated(const dfh_gn_problem *problem, const dfh_gn_frame *frame, const dfh_gn_normal_gate *gate,
                       const dfh_gn_solve_params *params, void *stream) {
    dfh::GatedAssocArgs ga;
    const int rc = check_fused_gated("dfh_gn_solve_gated", problem, frame, gate, &ga);
    if (rc != DFH_OK) return rc;
    return gn_solve_impl("dfh_gn_solve_gated", *problem, BuildAssoc{nullptr, nullptr, &ga}, params, stream);
}

int dfh_gn_solve_volume(const dfh_gn_problem *problem, const dfh_gn_volume_term *term, const dfh_gn_solve_params *params, void *stream) {
    dfh::VolAssocArgs va;
    const int rc = check_fused_volume("dfh_gn_solve_volume", problem, term, &va);
    if (rc != DFH_OK) return rc;
    return gn_solve_impl("dfh_gn_solve_volume", *problem, BuildAssoc{nullptr, &va}, params, stream);
}

}  // extern "C"
