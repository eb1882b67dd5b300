// Volume data term of the warp-field solve: corr / valid of the GN samples from a live TSDF VOLUME (dfh_gn_associate_volume).
//
// The projective association (dfh_solve.hip: associate_kernel) costs one projection + one depth pixel per sample and VIEW; the
// frame loop fuses all views into a live TSDF every frame anyway, and a volume-in caller (the reference's Fusion workflow,
// test.py: .dist files) has nothing else.  Against the volume a sample costs one trilinear cell whatever the number of views:
// warp the sample as associate_kernel does (same operations, same bits), read the cell's eight corners, and take one Newton
// step along the interpolant's gradient onto its zero level set.  Definition, operation by operation: include/dfusion_hip.h.
//
// One sample per lane, 256-thread workgroups, no LDS, no atomics: the workgroups are independent.  About 150 fp64 operations
// per sample against a chain of four dependent memory round trips (nbr / weights / position -> node_dq rows -> warp -> the
// cell's corners), so the kernel is bound by that chain's latency, not by registers or arithmetic.  What is done about it:
// every load of a link is requested before the first use of any of them (the k node rows together; the eight corners as four
// z-adjacent pairs, one 8- or 16-byte load each, together), lanes outside the grid read cell (0,0,0) instead of branching
// round the loads (no divergence, one exit), and the small footprint (no LDS; knn 4: 76 VGPRs) leaves the waves to hide the rest.
#include "dfh_dq.h"

#include <cmath>

namespace dfh {

struct VolAssocParams {
    DQ lw;
    double value_to_vox, band, max_dist2, min_grad2;   // max_dist2 <= 0: no gate
    int res[3];
};

// two z-adjacent voxels: the pair is only element-aligned (a cell starts at any z), which the load is told
template <typename LiveT>
struct LivePair { LiveT lo, hi; };

template <typename LiveT>
__device__ __forceinline__ LivePair<LiveT> load_pair(const LiveT *__restrict__ p) {
    LivePair<LiveT> v;
    __builtin_memcpy(&v, p, sizeof(v));                // one global_load_dwordx2 (float) / dwordx4 (double), alignment sizeof(LiveT)
    return v;
}

// K = knn as a compile-time constant: the k index / weight loads, then the k node rows, are each straight-line code (with a
// run-time k every neighbour slot is a branch of its own with a wait behind it: k + k dependent round trips instead of 1 + 1).
template <typename LiveT, int K>
__global__ __launch_bounds__(256) void associate_volume_kernel(const double *__restrict__ spos, const int *__restrict__ nbr,
                                                                const double *__restrict__ wts, int S,
                                                                const double *__restrict__ node_dq,
                                                                const LiveT *__restrict__ live, const VolAssocParams p,
                                                                double *__restrict__ corr, unsigned char *__restrict__ valid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    // 1. warp: associate_kernel's statements
    int idx[kBlendKMax];
    double w[kBlendKMax];
#pragma unroll
    for (int j = 0; j < kBlendKMax; ++j) {
        idx[j] = j < K ? nbr[(size_t)i * K + j] : 0;
        w[j] = j < K ? wts[(size_t)i * K + j] : 0.0;
    }
    const double px = spos[3 * (size_t)i], py = spos[3 * (size_t)i + 1], pz = spos[3 * (size_t)i + 2];
    // the K node rows, all requested together, then blended from registers (slot j = row j: blend_static's own arithmetic)
    double rows[8 * K];
    int slot[kBlendKMax];
#pragma unroll
    for (int j = 0; j < K; ++j) {
#pragma unroll
        for (int c = 0; c < 8; ++c) rows[8 * j + c] = node_dq[8 * (size_t)idx[j] + c];
    }
#pragma unroll
    for (int j = 0; j < kBlendKMax; ++j) slot[j] = j < K ? j : 0;
    double b[8];
    blend_static(rows, slot, w, K, b);
    const D3 x1 = dqb_warp_exact(b, round_f32(px), round_f32(py), round_f32(pz));
    const D3 xp = dqb_warp_exact(p.lw.q, round_f32(x1.x), round_f32(x1.y), round_f32(x1.z));
    // 2. in grid: decided on the doubles (NaN and +-inf fail the comparisons), before any conversion to int
    const bool in_grid = xp.x >= 0.0 && xp.x < (double)(p.res[0] - 1) && xp.y >= 0.0 && xp.y < (double)(p.res[1] - 1) &&
                         xp.z >= 0.0 && xp.z < (double)(p.res[2] - 1);
    const double X0 = in_grid ? xp.x : 0.0, X1 = in_grid ? xp.y : 0.0, X2 = in_grid ? xp.z : 0.0;   // (outside: cell (0,0,0), discarded)
    const double fl0 = floor(X0), fl1 = floor(X1), fl2 = floor(X2);
    const int i0 = (int)fl0, i1 = (int)fl1, i2 = (int)fl2;          // 0 <= ia <= res[a] - 2
    const double f0 = X0 - fl0, f1 = X1 - fl1, f2 = X2 - fl2;
    // 3. corners: the standard trilinear cell, four z-adjacent pairs, all requested before the first use
    const size_t sy = (size_t)p.res[2], sx = (size_t)p.res[1] * sy;
    const LiveT *cell = live + ((size_t)i0 * sx + (size_t)i1 * sy + (size_t)i2);
    const LivePair<LiveT> r00 = load_pair(cell), r01 = load_pair(cell + sy), r10 = load_pair(cell + sx), r11 = load_pair(cell + sx + sy);
    const double u000 = (double)r00.lo * p.value_to_vox, u001 = (double)r00.hi * p.value_to_vox;
    const double u010 = (double)r01.lo * p.value_to_vox, u011 = (double)r01.hi * p.value_to_vox;
    const double u100 = (double)r10.lo * p.value_to_vox, u101 = (double)r10.hi * p.value_to_vox;
    const double u110 = (double)r11.lo * p.value_to_vox, u111 = (double)r11.hi * p.value_to_vox;
    // 4. band (strict; a NaN corner fails)
    const bool in_band = fabs(u000) < p.band && fabs(u001) < p.band && fabs(u010) < p.band && fabs(u011) < p.band &&
                         fabs(u100) < p.band && fabs(u101) < p.band && fabs(u110) < p.band && fabs(u111) < p.band;
    // 5. value and gradient of the interpolant
    const double dz00 = u001 - u000, dz01 = u011 - u010, dz10 = u101 - u100, dz11 = u111 - u110;
    const double e00 = u000 + f2 * dz00, e01 = u010 + f2 * dz01, e10 = u100 + f2 * dz10, e11 = u110 + f2 * dz11;
    const double dy0 = e01 - e00, dy1 = e11 - e10;
    const double h0 = e00 + f1 * dy0, h1 = e10 + f1 * dy1;
    const double g0 = h1 - h0;
    const double s = h0 + f0 * g0;
    const double g1 = dy0 + f0 * (dy1 - dy0);
    const double m0 = dz00 + f1 * (dz01 - dz00), m1 = dz10 + f1 * (dz11 - dz10);
    const double g2 = m0 + f0 * (m1 - m0);
    // 6. gradient and gate (G > 0 always: t = s / G)
    const double G = (g0 * g0 + g1 * g1) + g2 * g2;
    bool ok = in_grid && in_band && G >= p.min_grad2 && G > 0.0;
    if (p.max_dist2 > 0.0) ok = ok && s * s <= p.max_dist2 * G;
    // 7. one Newton step onto the zero level set; the row is always written
    const double t = s / G;
    corr[3 * (size_t)i] = ok ? xp.x - t * g0 : 0.0;
    corr[3 * (size_t)i + 1] = ok ? xp.y - t * g1 : 0.0;
    corr[3 * (size_t)i + 2] = ok ? xp.z - t * g2 : 0.0;
    valid[i] = ok ? 1 : 0;
}

}  // namespace dfh

extern "C" int dfh_gn_associate_volume(const dfh_gn_problem *problem, const dfh_gn_volume_term *term, void *stream) {
    using namespace dfh;
    const char *what = "dfh_gn_associate_volume";
    DFH_REQUIRE(problem, "%s: null problem", what);
    DFH_REQUIRE(term, "%s: null volume term", what);
    const dfh_gn_problem &q = *problem;
    const dfh_gn_volume_term &v = *term;
    DFH_REQUIRE(q.n_samples >= 0 && q.n_nodes >= 1, "%s: bad sizes", what);
    DFH_REQUIRE(q.knn >= 1 && q.knn <= kBlendKMax, "%s: knn=%d outside [1,%d]", what, q.knn, kBlendKMax);
    DFH_REQUIRE(q.node_dq, "%s: null node_dq", what);
    if (q.n_samples > 0)                                                           // (normals are not read)
        DFH_REQUIRE(q.sample_pos && q.nbr && q.weights && q.corr && q.valid, "%s: null sample pointer", what);
    DFH_REQUIRE(v.live.data, "%s: null live volume", what);
    DFH_REQUIRE(v.live.dtype == DFH_F32 || v.live.dtype == DFH_F64, "%s: bad live dtype %d", what, v.live.dtype);
    DFH_REQUIRE(v.live.res[0] >= 2 && v.live.res[1] >= 2 && v.live.res[2] >= 2, "%s: bad grid %dx%dx%d (a cell needs 2 voxels per axis)",
                what, v.live.res[0], v.live.res[1], v.live.res[2]);
    DFH_REQUIRE(std::isfinite(v.value_to_vox) && v.value_to_vox != 0.0, "%s: value_to_vox must be finite and non-zero", what);
    DFH_REQUIRE(v.band > 0.0, "%s: band must be > 0", what);                       // (NaN fails)
    DFH_REQUIRE(v.min_grad >= 0.0, "%s: min_grad must be >= 0", what);             // (NaN fails)
    DFH_REQUIRE(!std::isnan(v.max_dist), "%s: max_dist is NaN", what);
    if (q.n_samples == 0) return DFH_OK;
    VolAssocParams p;
    for (int c = 0; c < 8; ++c) p.lw.q[c] = q.lw_dq[c];
    p.value_to_vox = v.value_to_vox;
    p.band = v.band;
    p.max_dist2 = v.max_dist > 0.0 ? v.max_dist * v.max_dist : 0.0;
    p.min_grad2 = v.min_grad * v.min_grad;
    for (int a = 0; a < 3; ++a) p.res[a] = v.live.res[a];
    const dim3 grid((q.n_samples + 255) / 256), block(256);
#define DFH_AV_LAUNCH(T, KK)                                                                                                   \
    case KK:                                                                                                                   \
        hipLaunchKernelGGL((associate_volume_kernel<T, KK>), grid, block, 0, (hipStream_t)stream, q.sample_pos, q.nbr, q.weights, \
                           q.n_samples, q.node_dq, static_cast<const T *>(v.live.data), p, q.corr, q.valid);                   \
        break;
#define DFH_AV_LAUNCH_K(T)                                                                                                     \
    switch (q.knn) {                                                                                                           \
        DFH_AV_LAUNCH(T, 1) DFH_AV_LAUNCH(T, 2) DFH_AV_LAUNCH(T, 3) DFH_AV_LAUNCH(T, 4)                                        \
        DFH_AV_LAUNCH(T, 5) DFH_AV_LAUNCH(T, 6) DFH_AV_LAUNCH(T, 7) DFH_AV_LAUNCH(T, 8)                                        \
    }
    if (v.live.dtype == DFH_F32) {
        DFH_AV_LAUNCH_K(float)
    } else {
        DFH_AV_LAUNCH_K(double)
    }
#undef DFH_AV_LAUNCH_K
#undef DFH_AV_LAUNCH
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}
