// What more than one stage of the warp-field solve uses and what depends on nothing else of it: the quaternion algebra and
// the reference's blend, the block lookup of the block-sparse rows, the 6x6 inverse and the twist update of one node.
// Device side only, everything fp64.
#pragma once
#include "dfh_dq.h"

namespace dfh {

constexpr int kKMaxS = 8;

struct Q4 { double w, x, y, z; };

__device__ __forceinline__ Q4 qmul(const Q4 &a, const Q4 &b) {
    Q4 o;
    o.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    o.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    o.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
    o.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
    return o;
}
__device__ __forceinline__ Q4 qconj(const Q4 &a) { return Q4{a.w, -a.x, -a.y, -a.z}; }
__device__ __forceinline__ Q4 qpure(double x, double y, double z) { return Q4{0.0, x, y, z}; }
__device__ __forceinline__ Q4 qadd(const Q4 &a, const Q4 &b) { return Q4{a.w + b.w, a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ Q4 qscale(const Q4 &a, double s) { return Q4{a.w * s, a.x * s, a.y * s, a.z * s}; }

// Blend the k node DQs of one point (explicit indices, weights from positions exactly like
// Fusion.dq_blend, core/fusion.py:527-551), then warp point (and normal) through the blend and
// m_lw like Fusion.warp (:502-520).  bh receives the normalised blend, wts the raw weights.
__device__ __forceinline__ void blend_from_indices(const double *__restrict__ node_dq, const double *__restrict__ node_pos,
                                                   const double *__restrict__ node_w, const int *idx, int k,
                                                   double px, double py, double pz, double *bh, double *nb_out,
                                                   double *wts) {
    double b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < kKMaxS; ++j) {
        if (j < k) {
            const int gi = idx[j];
            const double dx = px - node_pos[3 * gi], dy = py - node_pos[3 * gi + 1], dz = pz - node_pos[3 * gi + 2];
            const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
            const double t = dist / (2.0 * node_w[gi]);
            const double wgt = exp(-1.0 * (t * t));
            if (wts) wts[j] = wgt;
#pragma unroll
            for (int c = 0; c < 8; ++c) b[c] = b[c] + wgt * node_dq[8 * gi + c];
        }
    }
    const double n2 = ((b[0] * b[0] + b[1] * b[1]) + (b[2] * b[2] + b[3] * b[3])) +
                      ((b[4] * b[4] + b[5] * b[5]) + (b[6] * b[6] + b[7] * b[7]));
    const double n = sqrt(n2);
    if (n == 0.0) {
        bh[0] = 1.0;
#pragma unroll
        for (int c = 1; c < 8; ++c) bh[c] = 0.0;
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) bh[c] = b[c] / n;
    }
    if (nb_out) *nb_out = n;
}

// Block-sparse rows: node a owns blocks vals[row_ptr[a] .. row_ptr[a+1]) with sorted column
// nodes col[]; a block is 36 doubles, row-major 6x6.
__device__ __forceinline__ int find_block(const int *__restrict__ row_ptr, const int *__restrict__ col, int a, int b) {
    int lo = row_ptr[a], hi = row_ptr[a + 1] - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const int c = col[mid];
        if (c == b) return mid;
        if (c < b) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

// Row `r` (r = 0..5, may differ between lanes) of the same inverse, the same bits as inv6's row r, without the 36 outputs: the
// persistent PCG wants one row per lane and was spilling registers around the full inverse in its 1 024-thread form.
// (A^-1)[r][j] = sum_k Li[k][r] Li[k][j] over k >= max(r, j); Li[k][r] is picked from the k-th row with compares (no dynamic
// index), and is exactly 0 for k < r, so the sum may start at k = j: the extra terms add +0.0 to a +0.0.
__device__ __forceinline__ void inv6_row(const double *A, int r, double *row) {
    double L[6][6], Li[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) { L[i][j] = 0.0; Li[i][j] = 0.0; }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[6 * j + j];
#pragma unroll
        for (int k = 0; k < 6; ++k) if (k < j) d -= L[j][k] * L[j][k];
        d = d > 0.0 ? sqrt(d) : 1.0;
        L[j][j] = d;
        const double id = 1.0 / d;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if (i > j) {
                double v = A[6 * i + j];
#pragma unroll
                for (int k = 0; k < 6; ++k) if (k < j) v -= L[i][k] * L[j][k];
                L[i][j] = v * id;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if (i >= c) {
                double v = i == c ? 1.0 : 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) if (k >= c && k < i) v -= L[i][k] * Li[k][c];
                Li[i][c] = v / L[i][i];
            }
        }
    }
    double lr[6];                                               // Li[k][r]
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double v = Li[k][0];
#pragma unroll
        for (int c = 1; c < 6; ++c) v = r == c ? Li[k][c] : v;
        lr[k] = v;
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) if (k >= j) v += lr[k] * Li[k][j];
        row[j] = v;
    }
}

__device__ __forceinline__ void inv6(const double *A, double *Ainv) {
    // A = L L^T (SPD after damping), A^-1 = L^-T L^-1; every loop has compile-time bounds so the
    // 6x6 arrays live in registers.  A non-positive pivot (rank-deficient block) is replaced by 1:
    // the preconditioner only has to be SPD, not exact.
    double L[6][6], Li[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) { L[i][j] = 0.0; Li[i][j] = 0.0; }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[6 * j + j];
#pragma unroll
        for (int k = 0; k < 6; ++k) if (k < j) d -= L[j][k] * L[j][k];
        d = d > 0.0 ? sqrt(d) : 1.0;
        L[j][j] = d;
        const double id = 1.0 / d;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if (i > j) {
                double v = A[6 * i + j];
#pragma unroll
                for (int k = 0; k < 6; ++k) if (k < j) v -= L[i][k] * L[j][k];
                L[i][j] = v * id;
            }
        }
    }
    // Li = L^-1 (lower triangular), column by column
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if (i >= c) {
                double v = i == c ? 1.0 : 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) if (k >= c && k < i) v -= L[i][k] * Li[k][c];
                Li[i][c] = v / L[i][i];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) if (k >= i && k >= j) v += Li[k][i] * Li[k][j];
            Ainv[6 * i + j] = v;
        }
}

// dq <- exp(step * xi) (x) dq for one node (exp: rotation exp(omega), translation v; oracle/gn_np.py)
__device__ __forceinline__ void apply_twist_one(double *__restrict__ d, double ox, double oy, double oz, double vx, double vy, double vz) {
    const double th = sqrt(ox * ox + oy * oy + oz * oz);
    const double half = 0.5 * th;
    const double s = th < 1e-8 ? 0.5 - th * th / 48.0 : sin(half) / th;
    const Q4 q{cos(half), s * ox, s * oy, s * oz};
    const Q4 qe = qscale(qmul(qpure(vx, vy, vz), q), 0.5);
    const Q4 r{d[0], d[1], d[2], d[3]}, dd{d[4], d[5], d[6], d[7]};
    const Q4 nr = qmul(q, r);
    const Q4 nd = qadd(qmul(q, dd), qmul(qe, r));
    d[0] = nr.w; d[1] = nr.x; d[2] = nr.y; d[3] = nr.z;
    d[4] = nd.w; d[5] = nd.x; d[6] = nd.y; d[7] = nd.z;
}

}  // namespace dfh
