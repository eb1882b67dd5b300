// K25  mesh smoothing, Taubin's lambda|mu filter over a fixed Laplacian (dfh_mesh_smooth_*), and area-weighted vertex normals
// (dfh_mesh_vertex_normals).  No reference counterpart.  Every output is defined operation by operation in
// include/dfusion_hip.h and is a function of the mesh and the parameters alone; tests/smooth_np.py restates all of it and agrees
// bit for bit.
//
// Adjacency.  The caller sorts the 3F corner entries by the vertex they name (one stable torch.sort, the grouping K24 uses:
// plumbing).  Prepare writes, in that order, an int32 neighbour pair (a, b) per entry -- the two other corners of the entry's
// face, in the face's winding -- and where every vertex's list begins and ends.  The step then reads ONE contiguous list per
// vertex and never touches the face array.  The range rule is K24's ms_corner_ranges_kernel restated, not shared: that file is
// left as it is, so its device code is the parent's by construction.
// Operator.  Uniform: every entry weighs 1 (a neighbour counts once per face sharing the edge; on a closed manifold the umbrella
// operator exactly); nothing is stored.  Cotangent: an fp64 pair per entry, computed from the INPUT positions once.  The operator
// is fixed for the whole call: that makes lambda|mu a linear filter with Taubin's transfer function (1 - lam k)(1 - mu k) per
// iteration, and keeps square roots and divisions out of the step.  A negative cotangent (the angle opposite the edge is
// obtuse) is clamped to 0: with a negative weight x + factor * (L x) is no longer a combination of the neighbours that pulls
// towards them, the sum W of a vertex's weights can vanish or change sign, and a pass can push a vertex through its ring.
// Sum order.  One lane a vertex, the accumulators are registers, entries in ascending order from 0.0: no float atomic exists in
// this file and the only integer atomic is the error flag.
// Values.  Two fp64 ping-pong buffers in the workspace; float32 input is widened exactly and rounded once at the end.  Layout:
// rows of four doubles (32 bytes, one sector a neighbour) or planes (value k of vertex v at k V + v); the same bits either way,
// measured in profiles/r29_smooth.txt.
// Loops.  Every loop runs over a fixed index range read before it starts; a lane never waits for another lane.  A vertex of
// valence in the thousands is one long loop in one lane (and its boundary test is quadratic in the valence): correct, and slow
// only for that lane's wave.
// Indices.  Every index that addresses memory (a list's bounds, a neighbour, a corner entry) is range-checked where it is loaded;
// what fails is skipped, and prepare raises the flag for it.
#include <cmath>

#include "dfh_common.h"

namespace dfh {

constexpr int kSmBlock = 256;
constexpr long kSmMaxFaces = ((1l << 31) - 1) / 3;      // 3F corner entries are indexed with an int
constexpr size_t kSmAlign = 32;                         // a row of four doubles never straddles a sector

enum { kSmBadCoord = 1, kSmBadFace = 4, kSmBadOrder = 8 };

struct SmWork {                          // the caller's workspace, cut up
    int *hdr;                            // 4 words: word 2 is the flag
    int *corner_begin, *corner_end;      // V each
    unsigned char *boundary;             // V
    int2 *nbr;                           // 3F
    double2 *wts;                        // 3F
    double *buf[2];                      // 4 V each
};

static size_t sm_carve(SmWork *w, char *p, long V, long F) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char *q = p ? p + o : nullptr; o += (bytes + kSmAlign - 1) & ~(kSmAlign - 1); return q; };
    char *hdr = take(16), *cb = take((size_t)V * 4), *ce = take((size_t)V * 4), *bnd = take((size_t)V);
    char *nbr = take((size_t)F * 24), *wts = take((size_t)F * 48), *b0 = take((size_t)V * 32), *b1 = take((size_t)V * 32);
    if (w) *w = SmWork{(int *)hdr, (int *)cb, (int *)ce, (unsigned char *)bnd, (int2 *)nbr, (double2 *)wts, {(double *)b0, (double *)b1}};
    return o;
}

__device__ __forceinline__ bool sm_finite(double p) { return fabs(p) <= 1.7976931348623157e308; }

// ---- prepare ----------------------------------------------------------------------------------------------------------------
// one lane a sorted corner entry: the list bounds of the vertex it names, its neighbour pair, its cotangent pair
template <typename VT, bool COT>
__global__ __launch_bounds__(kSmBlock) void sm_entries_kernel(const VT *__restrict__ verts, long V, const int *__restrict__ faces, long n,
                                                              const int *__restrict__ sorted_vert, const long long *__restrict__ corner_order,
                                                              int *__restrict__ corner_begin, int *__restrict__ corner_end, int2 *__restrict__ nbr,
                                                              double2 *__restrict__ wts, int *__restrict__ bad) {
    const long i = (long)blockIdx.x * kSmBlock + threadIdx.x;
    if (i >= n) return;
    const int v = sorted_vert[i];
    int2 ab = make_int2(-1, -1);
    double2 w = make_double2(0.0, 0.0);
    if (v < 0 || v >= V) atomicOr(bad, kSmBadFace);
    else {
        if (i == 0 || sorted_vert[i - 1] != v) corner_begin[v] = (int)i;
        if (i == n - 1 || sorted_vert[i + 1] != v) corner_end[v] = (int)(i + 1);
        const long long e = corner_order[i];
        if (e < 0 || e >= n) atomicOr(bad, kSmBadOrder);
        else {
            const long f = (long)(e / 3);
            const int c = (int)(e - 3 * f);
            const int a = faces[3 * f + (c + 1) % 3], b = faces[3 * f + (c + 2) % 3];
            if (faces[e] != v) atomicOr(bad, kSmBadOrder);
            else if (a < 0 || a >= V || b < 0 || b >= V) atomicOr(bad, kSmBadFace);
            else {
                ab = make_int2(a, b);
                if (COT) {
                    double pv[3], pa[3], pb[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        pv[k] = (double)verts[3 * (long)v + k];
                        pa[k] = (double)verts[3 * (long)a + k];
                        pb[k] = (double)verts[3 * (long)b + k];
                    }
                    const double e1x = pa[0] - pv[0], e1y = pa[1] - pv[1], e1z = pa[2] - pv[2];
                    const double e2x = pb[0] - pv[0], e2y = pb[1] - pv[1], e2z = pb[2] - pv[2];
                    const double n0 = e1y * e2z - e1z * e2y, n1 = e1z * e2x - e1x * e2z, n2 = e1x * e2y - e1y * e2x;
                    const double A2 = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
                    if (A2 > 0.0) {
                        const double da = ((pv[0] - pb[0]) * (pa[0] - pb[0]) + (pv[1] - pb[1]) * (pa[1] - pb[1])) + (pv[2] - pb[2]) * (pa[2] - pb[2]);
                        const double db = ((pv[0] - pa[0]) * (pb[0] - pa[0]) + (pv[1] - pa[1]) * (pb[1] - pa[1])) + (pv[2] - pa[2]) * (pb[2] - pa[2]);
                        const double qa = da / A2, qb = db / A2;
                        w = make_double2(qa > 0.0 ? qa : 0.0, qb > 0.0 ? qb : 0.0);
                    }
                }
            }
        }
    }
    nbr[i] = ab;
    if (COT) wts[i] = w;
}

// one lane a vertex: its coordinates are finite; it is flagged when some other vertex is named by its list a number of times
// that is not 2 (an open edge 1, a non-manifold edge 3 or more, a repeated face 4).  Quadratic in the valence, exact.
template <typename VT>
__global__ __launch_bounds__(kSmBlock) void sm_boundary_kernel(const VT *__restrict__ verts, long V, long n, const int *__restrict__ corner_begin,
                                                               const int *__restrict__ corner_end, const int2 *__restrict__ nbr,
                                                               unsigned char *__restrict__ boundary, unsigned char *__restrict__ boundary_out,
                                                               int *__restrict__ bad) {
    const long v = (long)blockIdx.x * kSmBlock + threadIdx.x;
    if (v >= V) return;
    if (!(sm_finite((double)verts[3 * v]) && sm_finite((double)verts[3 * v + 1]) && sm_finite((double)verts[3 * v + 2]))) atomicOr(bad, kSmBadCoord);
    long i0 = corner_begin[v], i1 = corner_end[v];
    if (i0 < 0 || i1 > n || i0 > i1) i0 = i1 = 0;
    const int *__restrict__ ent = (const int *)nbr;          // the list as 2 (i1 - i0) neighbour entries
    bool flagged = false;
    for (long j = 2 * i0; j < 2 * i1 && !flagged; ++j) {
        const int u = ent[j];
        if (u == (int)v || u < 0) continue;
        int count = 0;
        for (long k = 2 * i0; k < 2 * i1; ++k) count += ent[k] == u;
        flagged = count != 2;
    }
    boundary[v] = flagged;
    if (boundary_out) boundary_out[v] = flagged;
}

// ---- values -----------------------------------------------------------------------------------------------------------------
template <int K, bool PLANES>
__device__ __forceinline__ void sm_load(const double *__restrict__ buf, long V, long v, double (&x)[K]) {
    if (PLANES) {
#pragma unroll
        for (int k = 0; k < K; ++k) x[k] = buf[(long)k * V + v];
    } else {
        const double2 *__restrict__ row = (const double2 *)(buf + 4 * v);
        if (K == 1) x[0] = buf[4 * v];
        else {
            const double2 lo = row[0];
            x[0] = lo.x; x[1] = lo.y;
            if (K > 2) {
                const double2 hi = row[1];
                x[2] = hi.x;
                if (K > 3) x[K - 1] = hi.y;
            }
        }
    }
}

template <int K, bool PLANES>
__device__ __forceinline__ void sm_store(double *__restrict__ buf, long V, long v, const double (&x)[K]) {
    if (PLANES) {
#pragma unroll
        for (int k = 0; k < K; ++k) buf[(long)k * V + v] = x[k];
    } else {
        double r[4] = {0.0, 0.0, 0.0, 0.0};                      // the whole row: a full sector, the unused slots 0
#pragma unroll
        for (int k = 0; k < K; ++k) r[k] = x[k];
        double2 *__restrict__ row = (double2 *)(buf + 4 * v);
        row[0] = make_double2(r[0], r[1]);
        row[1] = make_double2(r[2], r[3]);
    }
}

template <typename XT, int K, bool PLANES>
__global__ __launch_bounds__(kSmBlock) void sm_widen_kernel(const XT *__restrict__ x, long V, double *__restrict__ buf) {
    const long v = (long)blockIdx.x * kSmBlock + threadIdx.x;
    if (v >= V) return;
    double r[K];
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = (double)x[K * v + k];
    sm_store<K, PLANES>(buf, V, v, r);
}

template <typename XT, int K, bool PLANES>
__global__ __launch_bounds__(kSmBlock) void sm_narrow_kernel(const double *__restrict__ buf, long V, XT *__restrict__ out) {
    const long v = (long)blockIdx.x * kSmBlock + threadIdx.x;
    if (v >= V) return;
    double r[K];
    sm_load<K, PLANES>(buf, V, v, r);
#pragma unroll
    for (int k = 0; k < K; ++k) out[K * v + k] = (XT)r[k];
}

// ---- the step ---------------------------------------------------------------------------------------------------------------
// one lane a vertex: x' = x + factor * (sum over its entries of w_a (x_a - x) + w_b (x_b - x)) / W, in the list's order
template <int K, bool COT, bool PLANES>
__global__ __launch_bounds__(kSmBlock) void sm_step_kernel(const double *__restrict__ src, double *__restrict__ dst, long V, long n,
                                                           const int *__restrict__ corner_begin, const int *__restrict__ corner_end,
                                                           const int2 *__restrict__ nbr, const double2 *__restrict__ wts,
                                                           const unsigned char *__restrict__ fixed, double factor) {
    const long v = (long)blockIdx.x * kSmBlock + threadIdx.x;
    if (v >= V) return;
    double x[K], acc[K];
    sm_load<K, PLANES>(src, V, v, x);
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    long i0 = corner_begin[v], i1 = corner_end[v];
    if (i0 < 0 || i1 > n || i0 > i1) i0 = i1 = 0;
    double W = COT ? 0.0 : (double)(2 * (i1 - i0));
    // Two entries a trip, the next two pairs (and weights) loaded before this trip's rows are gathered: a lane's chain of dependent
    // round trips is one per two entries, not two per entry.  The sums take the entries one after the other all the same.  A
    // pair that fails its range check gathers the vertex's own row and adds nothing.
    const int2 none = make_int2(-1, -1);
    const double2 zero = make_double2(0.0, 0.0);
    int2 p0 = i0 < i1 ? nbr[i0] : none, p1 = i0 + 1 < i1 ? nbr[i0 + 1] : none;
    double2 q0 = COT && i0 < i1 ? wts[i0] : zero, q1 = COT && i0 + 1 < i1 ? wts[i0 + 1] : zero;
    for (long i = i0; i < i1; i += 2) {
        const int2 ab0 = p0, ab1 = p1;
        const double2 w0 = q0, w1 = q1;
        p0 = i + 2 < i1 ? nbr[i + 2] : none;
        p1 = i + 3 < i1 ? nbr[i + 3] : none;
        if (COT) {
            q0 = i + 2 < i1 ? wts[i + 2] : zero;
            q1 = i + 3 < i1 ? wts[i + 3] : zero;
        }
        const bool ok0 = ab0.x >= 0 && ab0.x < V && ab0.y >= 0 && ab0.y < V;
        const bool ok1 = i + 1 < i1 && ab1.x >= 0 && ab1.x < V && ab1.y >= 0 && ab1.y < V;
        double xa0[K], xb0[K], xa1[K], xb1[K];
        sm_load<K, PLANES>(src, V, ok0 ? ab0.x : v, xa0);
        sm_load<K, PLANES>(src, V, ok0 ? ab0.y : v, xb0);
        sm_load<K, PLANES>(src, V, ok1 ? ab1.x : v, xa1);
        sm_load<K, PLANES>(src, V, ok1 ? ab1.y : v, xb1);
        if (ok0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                acc[k] += COT ? w0.x * (xa0[k] - x[k]) : xa0[k] - x[k];      // (uniform: 1.0 * d is d)
                acc[k] += COT ? w0.y * (xb0[k] - x[k]) : xb0[k] - x[k];
            }
            if (COT) {
                W += w0.x;
                W += w0.y;
            }
        }
        if (ok1) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                acc[k] += COT ? w1.x * (xa1[k] - x[k]) : xa1[k] - x[k];
                acc[k] += COT ? w1.y * (xb1[k] - x[k]) : xb1[k] - x[k];
            }
            if (COT) {
                W += w1.x;
                W += w1.y;
            }
        }
    }
    if (W > 0.0 && !(fixed && fixed[v])) {
#pragma unroll
        for (int k = 0; k < K; ++k) x[k] = x[k] + factor * (acc[k] / W);
    }
    sm_store<K, PLANES>(dst, V, v, x);
}

// ---- vertex normals ---------------------------------------------------------------------------------------------------------
// one lane a vertex: the sum of (p_a - p_v) x (p_b - p_v) over its entries, in their order (area weighting), times sign, over its length
template <typename VT>
__global__ __launch_bounds__(kSmBlock) void sm_normals_kernel(const VT *__restrict__ verts, long V, long n, const int *__restrict__ corner_begin,
                                                              const int *__restrict__ corner_end, const int2 *__restrict__ nbr, double sign,
                                                              VT *__restrict__ normals) {
    const long v = (long)blockIdx.x * kSmBlock + threadIdx.x;
    if (v >= V) return;
    const double px = (double)verts[3 * v], py = (double)verts[3 * v + 1], pz = (double)verts[3 * v + 2];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    long i0 = corner_begin[v], i1 = corner_end[v];
    if (i0 < 0 || i1 > n || i0 > i1) i0 = i1 = 0;
    for (long i = i0; i < i1; ++i) {
        const int2 ab = nbr[i];
        if (ab.x < 0 || ab.x >= V || ab.y < 0 || ab.y >= V) continue;
        const double e1x = (double)verts[3 * (long)ab.x] - px, e1y = (double)verts[3 * (long)ab.x + 1] - py, e1z = (double)verts[3 * (long)ab.x + 2] - pz;
        const double e2x = (double)verts[3 * (long)ab.y] - px, e2y = (double)verts[3 * (long)ab.y + 1] - py, e2z = (double)verts[3 * (long)ab.y + 2] - pz;
        s0 += e1y * e2z - e1z * e2y;
        s1 += e1z * e2x - e1x * e2z;
        s2 += e1x * e2y - e1y * e2x;
    }
    s0 = sign * s0; s1 = sign * s1; s2 = sign * s2;
    const double len = sqrt((s0 * s0 + s1 * s1) + s2 * s2);
    const bool ok = len > 0.0;
    normals[3 * v] = (VT)(ok ? s0 / len : 0.0);
    normals[3 * v + 1] = (VT)(ok ? s1 / len : 0.0);
    normals[3 * v + 2] = (VT)(ok ? s2 / len : 0.0);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static unsigned sm_blocks(long n) { return (unsigned)((n + kSmBlock - 1) / kSmBlock); }

static bool sm_sizes_ok(long V, long F) { return V >= 0 && V < (1l << 31) && F >= 0 && F <= kSmMaxFaces; }

static int sm_check_sizes(const char *what, long V, long F) {
    DFH_REQUIRE(V >= 0 && V < (1l << 31), "%s: bad vertex count %ld", what, V);
    DFH_REQUIRE(F >= 0 && F <= kSmMaxFaces, "%s: bad face count %ld (3F must fit an int)", what, F);
    DFH_REQUIRE(F == 0 || V > 0, "%s: %ld faces of no vertices", what, F);
    return DFH_OK;
}

static int sm_check_work(const char *what, long V, long F, const void *workspace, size_t workspace_bytes) {
    DFH_REQUIRE(workspace, "%s: null workspace", what);
    DFH_REQUIRE(((size_t)workspace & (kSmAlign - 1)) == 0, "%s: the workspace is not 32-byte aligned", what);
    DFH_REQUIRE(workspace_bytes >= sm_carve(nullptr, nullptr, V, F), "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes,
                sm_carve(nullptr, nullptr, V, F));
    return DFH_OK;
}

template <typename VT>
static void sm_prepare_launch(const SmWork &w, const void *verts, long V, const int *faces, long F, const int *sorted_vert, const long long *corner_order,
                              bool cot, unsigned char *boundary_out, hipStream_t s) {
    const long n = 3 * F;
    if (F > 0) {
        if (cot)
            hipLaunchKernelGGL((sm_entries_kernel<VT, true>), dim3(sm_blocks(n)), dim3(kSmBlock), 0, s, (const VT *)verts, V, faces, n, sorted_vert,
                               corner_order, w.corner_begin, w.corner_end, w.nbr, w.wts, w.hdr + 2);
        else
            hipLaunchKernelGGL((sm_entries_kernel<VT, false>), dim3(sm_blocks(n)), dim3(kSmBlock), 0, s, (const VT *)verts, V, faces, n, sorted_vert,
                               corner_order, w.corner_begin, w.corner_end, w.nbr, w.wts, w.hdr + 2);
    }
    hipLaunchKernelGGL((sm_boundary_kernel<VT>), dim3(sm_blocks(V)), dim3(kSmBlock), 0, s, (const VT *)verts, V, n, (const int *)w.corner_begin,
                       (const int *)w.corner_end, (const int2 *)w.nbr, w.boundary, boundary_out, w.hdr + 2);
}

template <int K, bool COT, bool PLANES>
static void sm_run_launch(const SmWork &w, const void *x, int dtype, long V, long F, const unsigned char *fixed, int iters, double lam, double mu, void *out,
                          hipStream_t s) {
    const dim3 grid(sm_blocks(V)), block(kSmBlock);
    if (dtype == DFH_F32) hipLaunchKernelGGL((sm_widen_kernel<float, K, PLANES>), grid, block, 0, s, (const float *)x, V, w.buf[0]);
    else hipLaunchKernelGGL((sm_widen_kernel<double, K, PLANES>), grid, block, 0, s, (const double *)x, V, w.buf[0]);
    int cur = 0;
    for (int it = 0; it < iters; ++it) {
        for (int half = 0; half < 2; ++half) {
            if (half == 1 && mu == 0.0) continue;
            hipLaunchKernelGGL((sm_step_kernel<K, COT, PLANES>), grid, block, 0, s, (const double *)w.buf[cur], w.buf[cur ^ 1], V, 3 * F,
                               (const int *)w.corner_begin, (const int *)w.corner_end, (const int2 *)w.nbr, (const double2 *)w.wts, fixed,
                               half == 0 ? lam : mu);
            cur ^= 1;
        }
    }
    if (dtype == DFH_F32) hipLaunchKernelGGL((sm_narrow_kernel<float, K, PLANES>), grid, block, 0, s, (const double *)w.buf[cur], V, (float *)out);
    else hipLaunchKernelGGL((sm_narrow_kernel<double, K, PLANES>), grid, block, 0, s, (const double *)w.buf[cur], V, (double *)out);
}

template <int K>
static void sm_run_width(const SmWork &w, bool cot, bool planes, const void *x, int dtype, long V, long F, const unsigned char *fixed, int iters, double lam,
                         double mu, void *out, hipStream_t s) {
    if (cot && planes) sm_run_launch<K, true, true>(w, x, dtype, V, F, fixed, iters, lam, mu, out, s);
    else if (cot) sm_run_launch<K, true, false>(w, x, dtype, V, F, fixed, iters, lam, mu, out, s);
    else if (planes) sm_run_launch<K, false, true>(w, x, dtype, V, F, fixed, iters, lam, mu, out, s);
    else sm_run_launch<K, false, false>(w, x, dtype, V, F, fixed, iters, lam, mu, out, s);
}

}  // namespace dfh

using namespace dfh;

extern "C" size_t dfh_mesh_smooth_workspace_bytes(long n_verts, long n_faces) {
    if (!sm_sizes_ok(n_verts, n_faces)) return 0;
    return sm_carve(nullptr, nullptr, n_verts, n_faces);
}

extern "C" int dfh_mesh_smooth_prepare(const void *verts, int dtype, long n_verts, const int *faces, long n_faces, const int *sorted_corner_vert,
                                       const long long *corner_order, int weights, unsigned char *boundary_out, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    const char *what = "dfh_mesh_smooth_prepare";
    const long V = n_verts, F = n_faces;
    if (int rc = sm_check_sizes(what, V, F)) return rc;
    DFH_REQUIRE(dtype == DFH_F32 || dtype == DFH_F64, "%s: bad dtype %d", what, dtype);
    DFH_REQUIRE(weights == DFH_SMOOTH_UNIFORM || weights == DFH_SMOOTH_COTANGENT, "%s: bad weights %d", what, weights);
    DFH_REQUIRE(V == 0 || verts, "%s: null verts", what);
    DFH_REQUIRE(F == 0 || (faces && sorted_corner_vert && corner_order), "%s: null faces, sorted_corner_vert or corner_order", what);
    if (V == 0) return DFH_OK;
    if (int rc = sm_check_work(what, V, F, workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    SmWork w;
    sm_carve(&w, (char *)workspace, V, F);
    DFH_HIP_CHECK(hipMemsetAsync(w.hdr, 0, 16, s));
    DFH_HIP_CHECK(hipMemsetAsync(w.corner_begin, 0, (size_t)V * 4, s));
    DFH_HIP_CHECK(hipMemsetAsync(w.corner_end, 0, (size_t)V * 4, s));
    if (dtype == DFH_F32) sm_prepare_launch<float>(w, verts, V, faces, F, sorted_corner_vert, corner_order, weights == DFH_SMOOTH_COTANGENT, boundary_out, s);
    else sm_prepare_launch<double>(w, verts, V, faces, F, sorted_corner_vert, corner_order, weights == DFH_SMOOTH_COTANGENT, boundary_out, s);
    DFH_HIP_CHECK(hipGetLastError());
    int hdr[3] = {0, 0, 0};
    DFH_HIP_CHECK(hipMemcpyAsync(hdr, w.hdr, 12, hipMemcpyDeviceToHost, s));
    DFH_HIP_CHECK(hipStreamSynchronize(s));
    DFH_REQUIRE(!(hdr[2] & kSmBadCoord), "%s: a vertex coordinate is not finite", what);
    DFH_REQUIRE(!(hdr[2] & kSmBadFace), "%s: a face holds a vertex index outside [0, %ld)", what, V);
    DFH_REQUIRE(!(hdr[2] & kSmBadOrder), "%s: corner_order is not the order that sorts the corner entries into sorted_corner_vert", what);
    return DFH_OK;
}

extern "C" int dfh_mesh_smooth_run(const void *x, int dtype, long n_verts, long n_faces, long width, int weights, int boundary, int layout, int iters,
                                   double lam, double mu, void *out, void *workspace, size_t workspace_bytes, void *stream) {
    const char *what = "dfh_mesh_smooth_run";
    const long V = n_verts, F = n_faces;
    if (int rc = sm_check_sizes(what, V, F)) return rc;
    DFH_REQUIRE(dtype == DFH_F32 || dtype == DFH_F64, "%s: bad dtype %d", what, dtype);
    DFH_REQUIRE(width >= 1 && width <= 4, "%s: width must be 1 to 4, got %ld", what, width);
    DFH_REQUIRE(weights == DFH_SMOOTH_UNIFORM || weights == DFH_SMOOTH_COTANGENT, "%s: bad weights %d", what, weights);
    DFH_REQUIRE(boundary == DFH_SMOOTH_FIXED || boundary == DFH_SMOOTH_FREE, "%s: bad boundary %d", what, boundary);
    DFH_REQUIRE(layout == DFH_SMOOTH_ROWS || layout == DFH_SMOOTH_PLANES, "%s: bad layout %d", what, layout);
    DFH_REQUIRE(iters >= 0, "%s: iters must not be negative, got %d", what, iters);
    DFH_REQUIRE(std::isfinite(lam) && std::isfinite(mu), "%s: lam and mu must be finite, got %g and %g", what, lam, mu);
    DFH_REQUIRE(V == 0 || (x && out), "%s: null x or out", what);
    if (V == 0) return DFH_OK;
    if (int rc = sm_check_work(what, V, F, workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    SmWork w;
    sm_carve(&w, (char *)workspace, V, F);
    const unsigned char *fixed = boundary == DFH_SMOOTH_FIXED ? w.boundary : nullptr;
    const bool cot = weights == DFH_SMOOTH_COTANGENT, planes = layout == DFH_SMOOTH_PLANES;
    switch (width) {
        case 1: sm_run_width<1>(w, cot, planes, x, dtype, V, F, fixed, iters, lam, mu, out, s); break;
        case 2: sm_run_width<2>(w, cot, planes, x, dtype, V, F, fixed, iters, lam, mu, out, s); break;
        case 3: sm_run_width<3>(w, cot, planes, x, dtype, V, F, fixed, iters, lam, mu, out, s); break;
        default: sm_run_width<4>(w, cot, planes, x, dtype, V, F, fixed, iters, lam, mu, out, s); break;
    }
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

extern "C" int dfh_mesh_vertex_normals(const void *verts, int dtype, long n_verts, long n_faces, double sign, void *normals, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    const char *what = "dfh_mesh_vertex_normals";
    const long V = n_verts, F = n_faces;
    if (int rc = sm_check_sizes(what, V, F)) return rc;
    DFH_REQUIRE(dtype == DFH_F32 || dtype == DFH_F64, "%s: bad dtype %d", what, dtype);
    DFH_REQUIRE(std::isfinite(sign), "%s: sign must be finite, got %g", what, sign);
    DFH_REQUIRE(V == 0 || (verts && normals), "%s: null verts or normals", what);
    if (V == 0) return DFH_OK;
    if (int rc = sm_check_work(what, V, F, workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    SmWork w;
    sm_carve(&w, (char *)workspace, V, F);
    if (dtype == DFH_F32)
        hipLaunchKernelGGL((sm_normals_kernel<float>), dim3(sm_blocks(V)), dim3(kSmBlock), 0, s, (const float *)verts, V, 3 * F, (const int *)w.corner_begin,
                           (const int *)w.corner_end, (const int2 *)w.nbr, sign, (float *)normals);
    else
        hipLaunchKernelGGL((sm_normals_kernel<double>), dim3(sm_blocks(V)), dim3(kSmBlock), 0, s, (const double *)verts, V, 3 * F, (const int *)w.corner_begin,
                           (const int *)w.corner_end, (const int2 *)w.nbr, sign, (double *)normals);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}
