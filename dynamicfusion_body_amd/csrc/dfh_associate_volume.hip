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
#include "dfh_assoc_volume.h"

namespace dfh {

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
    // 2-7. the cell (dfh_assoc_volume.h); the row is always written
    double c[3];
    const bool ok = associate_volume_cell<LiveT>(live, p, xp, c);
    corr[3 * (size_t)i] = c[0];
    corr[3 * (size_t)i + 1] = c[1];
    corr[3 * (size_t)i + 2] = c[2];
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
    const int rc = check_volume_term(what, term, false);
    if (rc != DFH_OK) return rc;
    if (q.n_samples == 0) return DFH_OK;
    const VolAssocParams p = vol_assoc_params(q, v);
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
