// K3 front end, shared by the volume -> volume fusion (dfh_fuse_volume.hip) and the depth -> canonical fusion through the warp
// field (dfh_integrate_warped.hip): the brick shape and the parameter block, the stable k-nearest insertion, the LDS-staged node
// search of a brick, the Gaussian blend weights and the blended double warp of Fusion.warp (reference core/fusion.py:502-551), and
// the host helpers that size the per-brick candidate lists.  One statement of each: both callers' bits are the same by construction.
#pragma once
#include "dfh_dq.h"

namespace dfh {

constexpr int kBX = 4, kBY = 4, kBZ = 16;      // brick = one 256-thread block, z fastest (64-B rows)
constexpr int kCap = 256;                       // candidate nodes kept per brick (<= 256: one per thread when staged)
constexpr int kKMax = 8;                        // knn <= 8

struct DqbParams {
    DQ lw;
    double tdist, wmax;
    int X, Y, Z;
    int LX, LY, LZ;
    int x0, nx;
    int N, k;
    int nbx, nby, nbz;      // bricks per axis (over the slab)
};

// sorted (ascending, stable) insertion into a KS-slot list held in registers
template <int KS>
__device__ __forceinline__ void topk_insert(double (&bd)[KS], int (&bi)[KS], double d2, int idx) {
    bool ins = false;                       // once inserted, everything below shifts down: equal distances keep their
#pragma unroll
    for (int i = 0; i < KS; ++i) {          // arrival order (a stable sort, KD-tree-like: ties go to the lower node index)
        const bool lt = ins || d2 < bd[i];
        ins = lt;
        const double td = bd[i];
        const int ti = bi[i];
        bd[i] = lt ? d2 : td;
        bi[i] = lt ? idx : ti;
        d2 = lt ? td : d2;
        idx = lt ? ti : idx;
    }
}

template <int KS>
__device__ __forceinline__ double select_k(const double (&bd)[KS], int k) {
    double r = bd[0];
#pragma unroll
    for (int i = 1; i < KS; ++i) r = (k - 1 == i) ? bd[i] : r;
    return r;
}

// k nearest nodes of `pos` (ascending distance, ties by node index = stable argsort of the
// squared distances; what KDTree.query(pos, k+1)[1][:-1] yields, core/fusion.py:175-176).
// All 256 threads of the block must call this (LDS staging + barriers).
template <int KS>
__device__ __forceinline__ void block_knn(const double *__restrict__ node_pos, const int *__restrict__ c, int N,
                                          double px, double py, double pz, bool active,
                                          double (&bd)[KS], int (&bi)[KS]) {
    __shared__ double spos[kCap * 3];
    __shared__ int sidx[kCap];
    const int cnt = c[0];
    const int total = cnt >= 0 ? cnt : N;
#pragma unroll
    for (int i = 0; i < KS; ++i) { bd[i] = __builtin_huge_val(); bi[i] = -1; }
    for (int base = 0; base < total; base += kCap) {
        const int n = min(kCap, total - base);
        if ((int)threadIdx.x < n) {
            const int gi = cnt >= 0 ? c[1 + base + threadIdx.x] : base + (int)threadIdx.x;
            sidx[threadIdx.x] = gi;
            spos[3 * threadIdx.x + 0] = node_pos[3 * gi + 0];
            spos[3 * threadIdx.x + 1] = node_pos[3 * gi + 1];
            spos[3 * threadIdx.x + 2] = node_pos[3 * gi + 2];
        }
        __syncthreads();
        if (active) {
            for (int i = 0; i < n; ++i) {
                const double dx = px - spos[3 * i], dy = py - spos[3 * i + 1], dz = pz - spos[3 * i + 2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < bd[KS - 1]) topk_insert<KS>(bd, bi, d2, sidx[i]);
            }
        }
        __syncthreads();
    }
}

// Fusion.dq_blend + warp (core/fusion.py:502-551) for one point whose k nearest nodes are
// (bd, bi).  Returns the point warped by the blended DQ and then by m_lw (x1 is re-rounded to
// float32 inside the second dqb_warp, core/util.py:69); *wi_out = mean node distance (:180-183).
template <int KS>
__device__ __forceinline__ void dqb_weights(const double *__restrict__ node_w, const double (&bd)[KS], const int (&bi)[KS], int k,
                                            double (&wg)[KS], double &wi) {
    wi = 0.0;
#pragma unroll
    for (int j = 0; j < KS; ++j) {
        wg[j] = 0.0;
        if (j < k) {
            const double dist = sqrt(bd[j]);
            const double t = dist / (2.0 * node_w[bi[j]]);
            wg[j] = exp(-1.0 * (t * t));                                 // :537
            wi = wi + dist / (double)k;                                  // mean node distance (:180-183)
        }
    }
}

template <int KS>
__device__ __forceinline__ D3 dqb_blend_warp(const double *__restrict__ node_dq, const double (&wg)[KS], const int (&bi)[KS], int k,
                                             const double *lw, double px, double py, double pz) {
    double b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < KS; ++j) {
        if (j < k) {
            const int gi = bi[j];
#pragma unroll
            for (int c = 0; c < 8; ++c) b[c] = b[c] + wg[j] * node_dq[8 * gi + c];   // :538
        }
    }
    // 8-norm (:551), pairwise like numpy's reduction of 8 contiguous values
    const double n2 = ((b[0] * b[0] + b[1] * b[1]) + (b[2] * b[2] + b[3] * b[3])) +
                      ((b[4] * b[4] + b[5] * b[5]) + (b[6] * b[6] + b[7] * b[7]));
    const double n = sqrt(n2);
    if (n == 0.0) {                                                       // :544-549
        b[0] = 1.0;
#pragma unroll
        for (int c = 1; c < 8; ++c) b[c] = 0.0;
    } else {
        const double inv = 1.0 / n;                  // one division; each component within 1 ulp of b/n
#pragma unroll
        for (int c = 0; c < 8; ++c) b[c] = b[c] * inv;
    }
    const D3 x1 = dqb_warp_exact(b, px, py, pz);                          // :510
    return dqb_warp_exact(lw, round_f32(x1.x), round_f32(x1.y), round_f32(x1.z));   // :512
}

// The grid, live-grid and slab fields of a K2 / K3 parameter block (live_res == nullptr: calls that sample no live volume).
template <typename Params>
static void set_grid(Params &p, const dfh_slab &sl, const int *live_res) {
    p.X = sl.res[0]; p.Y = sl.res[1]; p.Z = sl.res[2];
    if (live_res) { p.LX = live_res[0]; p.LY = live_res[1]; p.LZ = live_res[2]; }
    p.x0 = sl.x0; p.nx = sl.x1 - sl.x0;
}

// ... and K3's node counts and bricks per axis on top (everything but lw, tdist and wmax)
static DqbParams dqb_params(const dfh_slab &sl, const int *live_res, int n_nodes, int knn) {
    DqbParams p = {};
    set_grid(p, sl, live_res);
    p.N = n_nodes; p.k = knn;
    p.nbx = (p.nx + kBX - 1) / kBX;
    p.nby = (p.Y + kBY - 1) / kBY;
    p.nbz = (p.Z + kBZ - 1) / kBZ;
    return p;
}

static size_t cand_bytes(const dfh_slab &sl) {
    const DqbParams p = dqb_params(sl, nullptr, 0, 0);
    return (((size_t)p.nbx * p.nby * p.nbz * (kCap + 1) * sizeof(int)) + 15) & ~(size_t)15;
}

}  // namespace dfh
