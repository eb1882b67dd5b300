// K24  mesh simplification by vertex clustering with quadric error metrics (dfh_mesh_simplify_*): the vertices of a triangle
// mesh are grouped by the cell of a uniform grid they lie in, every cluster is replaced by one representative (the regularised
// minimiser of its summed face-plane quadric, or its mean), the faces are remapped, the collapsed and the repeated ones dropped.
// No reference counterpart.  Every output is defined operation by operation in include/dfusion_hip.h and is a function of the
// mesh and the parameters alone; tests/simplify_np.py restates all of it and agrees bit for bit.
//
// Grouping.  The caller sorts: a stable sort of the int64 cell keys gives the vertices by cell and, inside a cell, by ascending
// index; a stable sort of the 3F corner entries by the vertex they name gives every vertex its (face, corner) list in ascending
// face then corner order.  Both are torch.sort in mesh.py (plumbing, as graph.py's).  Everything else is here.
// Sum order, two levels.  Q_v is added up per vertex over its corner list, Q_C per cluster over its members' Q_v, both from 0.0 in
// ascending order, one lane a vertex and one lane a cluster: the accumulators are registers, no float atomic exists in this file
// and the only integer atomics are the error flag, the fall-back count and the face-group counters and cursors, whose landing
// order shows in no output (the group lists are filled in any order and only searched for a lower face index).
// Cluster ids.  The first vertex of every key segment is the cluster's lowest index (the sort is stable): a flag at that vertex,
// a scan of the flags over the vertices (dfh_scan.h's two-level pair) and the id is the flagged vertices in front of it.
// Faces.  Remap, drop a face with two equal corners, group the rest by their lowest cluster id (count -> scan -> fill), and a face
// is a repeat when its group holds a lower face index with the same (middle, highest) pair.  Compaction of clusters and faces is
// flag -> scan -> emit.
// Loops.  Every loop runs over a fixed index range read before it starts (a segment of the sorted keys, a corner list, a member
// list, a face group); a lane never waits for another lane.  A cell with thousands of members or a vertex of valence in the
// thousands is one long loop in one lane: correct, and slow only for that lane's wave.
// Indices.  Every index that addresses memory (a face's corners, an entry of the two sort orders, a cluster id, a segment) is
// range-checked where it is loaded; what fails the check is skipped and raises the flag where a call reports one.
#include <cmath>

#include "dfh_common.h"
#include "dfh_scan.h"

namespace dfh {

constexpr int kMsBlock = 256;
constexpr int kMsWaves = kMsBlock / kWave;
constexpr int kMsScanChunk = 4 * kMsBlock;
constexpr long kMsMaxFaces = ((1l << 31) - 1) / 3;      // 3F corner entries are indexed with an int
constexpr double kMsCellLimit = 2097152.0;              // 2^21 cells an axis: three of them fill 63 bits of the key
static_assert(kMsScanChunk == 1024, "prefixes are chunk_base[e >> 10] + local[e]");

enum { kMsBadCoord = 1, kMsBadCell = 2, kMsBadFace = 4, kMsBadOrder = 8 };

struct MsWork {                          // the caller's workspace, cut up (N = max(V, F) + 1)
    int *hdr;                            // 4 words: cluster count / kept clusters, kept faces, the flag
    int *cnt, *local, *cur, *flag;       // N each
    int *chunk_tot, *chunk_base;         // N / 1024 + 2
    int *fmin, *fmid, *fmax, *glist;     // F each
    int *ref;                            // V
    double *qv;                          // 10 V, quadric k of vertex v at qv[k V + v]
};

static size_t ms_align8(size_t b) { return (b + 7) & ~(size_t)7; }

static size_t ms_carve(MsWork *w, char *p, long V, long F) {
    const size_t N = (size_t)(V > F ? V : F) + 1, nch = N / kMsScanChunk + 2;
    size_t o = 0;
    auto take = [&](size_t bytes) { char *q = p ? p + o : nullptr; o += ms_align8(bytes); return q; };
    char *hdr = take(16), *cnt = take(N * 4), *local = take(N * 4), *cur = take(N * 4), *flag = take(N * 4), *ct = take(nch * 4), *cb = take(nch * 4);
    char *fmin = take((size_t)F * 4), *fmid = take((size_t)F * 4), *fmax = take((size_t)F * 4), *glist = take((size_t)F * 4);
    char *ref = take((size_t)V * 4), *qv = take((size_t)V * 80);
    if (w) *w = MsWork{(int *)hdr, (int *)cnt, (int *)local, (int *)cur, (int *)flag, (int *)ct, (int *)cb, (int *)fmin, (int *)fmid, (int *)fmax,
                       (int *)glist, (int *)ref, (double *)qv};
    return o;
}

__device__ __forceinline__ int ms_prefix(const int *__restrict__ local, const int *__restrict__ chunk_base, int e) {
    return chunk_base[e >> 10] + local[e];
}

// the centre of the cell a key names: origin + (c + 0.5) * cell per axis (c + 0.5 is exact, one product, one sum)
struct MsGrid { double cell, o0, o1, o2; };

__device__ __forceinline__ void ms_centre(long long key, const MsGrid &g, double (&ctr)[3]) {
    const long long k = key < 0 ? 0 : key;
    ctr[0] = g.o0 + ((double)(k >> 42) + 0.5) * g.cell;
    ctr[1] = g.o1 + ((double)((k >> 21) & 0x1fffff) + 0.5) * g.cell;
    ctr[2] = g.o2 + ((double)(k & 0x1fffff) + 0.5) * g.cell;
}

// ---- keys -------------------------------------------------------------------------------------------------------------------
template <typename VT>
__global__ __launch_bounds__(kMsBlock) void ms_keys_kernel(const VT *__restrict__ verts, long V, const int *__restrict__ faces, long F, MsGrid g,
                                                           long long *__restrict__ keys, int *__restrict__ bad) {
    const long i = (long)blockIdx.x * kMsBlock + threadIdx.x;
    if (i < V) {
        const double o[3] = {g.o0, g.o1, g.o2};
        long long key = 0;
        int why = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double p = (double)verts[3 * i + a];
            const double q = floor((p - o[a]) / g.cell);
            if (!(fabs(p) <= 1.7976931348623157e308)) why |= kMsBadCoord;
            else if (!(q >= 0.0 && q < kMsCellLimit)) why |= kMsBadCell;
            else key = (key << 21) | (long long)q;
        }
        keys[i] = why ? -1ll : key;
        if (why) atomicOr(bad, why);
    }
    if (i < F) {
        const int a = faces[3 * i], b = faces[3 * i + 1], c = faces[3 * i + 2];
        if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) atomicOr(bad, kMsBadFace);
    }
}

// ---- grouping ---------------------------------------------------------------------------------------------------------------
// a flag at the lowest vertex of every key segment
__global__ __launch_bounds__(kMsBlock) void ms_heads_kernel(const long long *__restrict__ skeys, const long long *__restrict__ order, long V,
                                                            int *__restrict__ is_first, int *__restrict__ bad) {
    const long i = (long)blockIdx.x * kMsBlock + threadIdx.x;
    if (i >= V) return;
    const long long v = order[i];
    if (v < 0 || v >= V) {
        atomicOr(bad, kMsBadOrder);
        return;
    }
    if (i == 0 || skeys[i - 1] != skeys[i]) is_first[v] = 1;
}

// the lane of a segment's first position names the cluster and walks its members
__global__ __launch_bounds__(kMsBlock) void ms_segments_kernel(const long long *__restrict__ skeys, const long long *__restrict__ order, long V,
                                                               const int *__restrict__ local, const int *__restrict__ chunk_base,
                                                               int *__restrict__ vert_cluster, int *__restrict__ cluster_start,
                                                               int *__restrict__ cluster_count) {
    const long i = (long)blockIdx.x * kMsBlock + threadIdx.x;
    if (i >= V) return;
    const long long key = skeys[i];
    if (i > 0 && skeys[i - 1] == key) return;
    const long long first = order[i];
    if (first < 0 || first >= V) return;
    const int c = ms_prefix(local, chunk_base, (int)first);
    long j = i;
    for (; j < V && skeys[j] == key; ++j) {
        const long long v = order[j];
        if (v >= 0 && v < V) vert_cluster[v] = c;
    }
    cluster_start[c] = (int)i;
    cluster_count[c] = (int)(j - i);
}

// the corner entries sorted by the vertex they name: where each vertex's list begins and ends
__global__ __launch_bounds__(kMsBlock) void ms_corner_ranges_kernel(const int *__restrict__ sorted_vert, long n, long V, int *__restrict__ corner_begin,
                                                                    int *__restrict__ corner_end, int *__restrict__ bad) {
    const long i = (long)blockIdx.x * kMsBlock + threadIdx.x;
    if (i >= n) return;
    const int v = sorted_vert[i];
    if (v < 0 || v >= V) {
        atomicOr(bad, kMsBadFace);
        return;
    }
    if (i == 0 || sorted_vert[i - 1] != v) corner_begin[v] = (int)i;
    if (i == n - 1 || sorted_vert[i + 1] != v) corner_end[v] = (int)(i + 1);
}

// ---- quadrics ---------------------------------------------------------------------------------------------------------------
// one lane a vertex: Q_v over its corner list, in the list's order
template <typename VT>
__global__ __launch_bounds__(kMsBlock) void ms_vertex_quadric_kernel(const VT *__restrict__ verts, long V, const int *__restrict__ faces, long F, MsGrid g,
                                                                     const long long *__restrict__ keys, const long long *__restrict__ corner_order,
                                                                     const int *__restrict__ corner_begin, const int *__restrict__ corner_end,
                                                                     double *__restrict__ qv) {
    const long v = (long)blockIdx.x * kMsBlock + threadIdx.x;
    if (v >= V) return;
    double ctr[3];
    ms_centre(keys[v], g, ctr);
    double q[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) q[k] = 0.0;
    long i0 = corner_begin[v], i1 = corner_end[v];
    if (i0 < 0 || i1 > 3 * F || i0 > i1) i0 = i1 = 0;
    for (long i = i0; i < i1; ++i) {
        const long long e = corner_order[i];
        if (e < 0 || e >= 3 * F) continue;
        const long f = (long)(e / 3);
        const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
        if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) continue;
        const double ax = (double)verts[3 * (long)ia], ay = (double)verts[3 * (long)ia + 1], az = (double)verts[3 * (long)ia + 2];
        const double e1x = (double)verts[3 * (long)ib] - ax, e1y = (double)verts[3 * (long)ib + 1] - ay, e1z = (double)verts[3 * (long)ib + 2] - az;
        const double e2x = (double)verts[3 * (long)ic] - ax, e2y = (double)verts[3 * (long)ic + 1] - ay, e2z = (double)verts[3 * (long)ic + 2] - az;
        const double n0 = e1y * e2z - e1z * e2y, n1 = e1z * e2x - e1x * e2z, n2 = e1x * e2y - e1y * e2x;
        const double q0 = ax - ctr[0], q1 = ay - ctr[1], q2 = az - ctr[2];
        const double d = -((n0 * q0 + n1 * q1) + n2 * q2);
        q[0] += n0 * n0; q[1] += n0 * n1; q[2] += n0 * n2; q[3] += n1 * n1; q[4] += n1 * n2; q[5] += n2 * n2;
        q[6] += d * n0; q[7] += d * n1; q[8] += d * n2; q[9] += d * d;
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) qv[(long)k * V + v] = q[k];
}

// one lane a cluster: the mean, Q_C, the solve (LDL^T, the order of the header), the position, the fall-back count
template <typename VT>
__global__ __launch_bounds__(kMsBlock) void ms_cluster_kernel(const VT *__restrict__ verts, long V, MsGrid g, int mode, double reg,
                                                              const long long *__restrict__ keys, const long long *__restrict__ order,
                                                              const int *__restrict__ cluster_start, const int *__restrict__ cluster_count, long C,
                                                              const double *__restrict__ qv, VT *__restrict__ out, int *__restrict__ n_fallback) {
    const long c = (long)blockIdx.x * kMsBlock + threadIdx.x;
    bool fell = false;
    if (c < C) {
        long s = cluster_start[c], n = cluster_count[c];
        if (s < 0 || n < 0 || s + n > V) s = n = 0;
        double ctr[3] = {0.0, 0.0, 0.0}, S[3] = {0.0, 0.0, 0.0}, Q[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) Q[k] = 0.0;
        for (long j = 0; j < n; ++j) {
            const long long v = order[s + j];
            if (v < 0 || v >= V) continue;
            if (j == 0) ms_centre(keys[v], g, ctr);
#pragma unroll
            for (int a = 0; a < 3; ++a) S[a] += (double)verts[3 * v + a] - ctr[a];
            if (mode == DFH_SIMPLIFY_QUADRIC) {
#pragma unroll
                for (int k = 0; k < 10; ++k) Q[k] += qv[(long)k * V + v];
            }
        }
        const double cnt = (double)n;
        const double m[3] = {S[0] / cnt, S[1] / cnt, S[2] / cnt};
        double x[3] = {m[0], m[1], m[2]};
        if (mode == DFH_SIMPLIFY_QUADRIC) {
            fell = true;
            const double t = (Q[0] + Q[3]) + Q[5];
            if (t > 0.0) {
                const double lam = reg * t;
                const double M00 = Q[0] + lam, M10 = Q[1], M20 = Q[2], M11 = Q[3] + lam, M21 = Q[4], M22 = Q[5] + lam;
                const double r0 = lam * m[0] - Q[6], r1 = lam * m[1] - Q[7], r2 = lam * m[2] - Q[8];
                const double d0 = M00;
                if (d0 > 0.0) {
                    const double l10 = M10 / d0, l20 = M20 / d0;
                    const double d1 = M11 - l10 * M10;
                    if (d1 > 0.0) {
                        const double t21 = M21 - l20 * M10;
                        const double l21 = t21 / d1;
                        const double d2 = (M22 - l20 * M20) - l21 * t21;
                        if (d2 > 0.0) {
                            const double y0 = r0, y1 = r1 - l10 * y0, y2 = (r2 - l20 * y0) - l21 * y1;
                            const double x2 = y2 / d2;
                            const double x1 = y1 / d1 - l21 * x2;
                            const double x0 = (y0 / d0 - l10 * x1) - l20 * x2;
                            const double half = 0.5 * g.cell;
                            if (fabs(x0) <= half && fabs(x1) <= half && fabs(x2) <= half) {
                                x[0] = x0; x[1] = x1; x[2] = x2;
                                fell = false;
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) out[3 * c + a] = (VT)(ctr[a] + x[a]);
    }
    const int fallen = __popcll(__ballot(fell));
    if ((threadIdx.x & 63) == 0 && fallen) atomicAdd(n_fallback, fallen);
}

// one lane an output element: attribute k of cluster c = the fp64 sum over the members in their order, over the count
template <typename AT>
__global__ __launch_bounds__(kMsBlock) void ms_attr_kernel(const AT *__restrict__ attr, long V, long K, const long long *__restrict__ order,
                                                           const int *__restrict__ cluster_start, const int *__restrict__ cluster_count, long C,
                                                           AT *__restrict__ out) {
    const long i = (long)blockIdx.x * kMsBlock + threadIdx.x;
    if (i >= C * K) return;
    const long c = i / K, k = i - c * K;
    long s = cluster_start[c], n = cluster_count[c];
    if (s < 0 || n < 0 || s + n > V) s = n = 0;
    double sum = 0.0;
    for (long j = 0; j < n; ++j) {
        const long long v = order[s + j];
        if (v >= 0 && v < V) sum += (double)attr[v * K + k];
    }
    out[i] = (AT)(sum / (double)n);
}

// ---- faces ------------------------------------------------------------------------------------------------------------------
// remap and order a face's cluster ids; a face with two equal ids (or a bad index) belongs to no group
__global__ __launch_bounds__(kMsBlock) void ms_face_remap_kernel(const int *__restrict__ faces, long F, long V, const int *__restrict__ vert_cluster, long C,
                                                                 int *__restrict__ fmin, int *__restrict__ fmid, int *__restrict__ fmax,
                                                                 int *__restrict__ gcnt, int *__restrict__ bad) {
    const long f = (long)blockIdx.x * kMsBlock + threadIdx.x;
    if (f >= F) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    int lo = -1, mid = -1, hi = -1;
    if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) atomicOr(bad, kMsBadFace);
    else {
        const int ca = vert_cluster[a], cb = vert_cluster[b], cc = vert_cluster[c];
        if (ca < 0 || ca >= C || cb < 0 || cb >= C || cc < 0 || cc >= C) atomicOr(bad, kMsBadOrder);
        else if (ca != cb && cb != cc && ca != cc) {
            lo = min(ca, min(cb, cc));
            hi = max(ca, max(cb, cc));
            mid = ca ^ cb ^ cc ^ lo ^ hi;
            atomicAdd(gcnt + lo, 1);
        }
    }
    fmin[f] = lo; fmid[f] = mid; fmax[f] = hi;
}

__global__ __launch_bounds__(kMsBlock) void ms_group_fill_kernel(long F, const int *__restrict__ fmin, const int *__restrict__ local,
                                                                 const int *__restrict__ chunk_base, int *__restrict__ cursor, int *__restrict__ glist) {
    const long f = (long)blockIdx.x * kMsBlock + threadIdx.x;
    if (f >= F) return;
    const int lo = fmin[f];
    if (lo < 0) return;
    const long pos = (long)ms_prefix(local, chunk_base, lo) + atomicAdd(cursor + lo, 1);
    if (pos < F) glist[pos] = (int)f;                        // (always: the groups hold at most the faces)
}

// a face survives unless its group holds a lower face with the same (middle, highest) ids; survivors mark their clusters
__global__ __launch_bounds__(kMsBlock) void ms_face_keep_kernel(long F, const int *__restrict__ fmin, const int *__restrict__ fmid, const int *__restrict__ fmax,
                                                                const int *__restrict__ gcnt, const int *__restrict__ local, const int *__restrict__ chunk_base,
                                                                const int *__restrict__ glist, int *__restrict__ keep, int *__restrict__ ref) {
    const long f = (long)blockIdx.x * kMsBlock + threadIdx.x;
    if (f >= F) return;
    const int lo = fmin[f];
    bool k = lo >= 0;
    if (k) {
        const int mid = fmid[f], hi = fmax[f];
        const long at = ms_prefix(local, chunk_base, lo);
        const int n = gcnt[lo];
        for (int i = 0; i < n && at + i < F; ++i) {
            const int o = glist[at + i];
            if (o >= 0 && o < f && fmid[o] == mid && fmax[o] == hi) {
                k = false;
                break;
            }
        }
        if (k) { ref[lo] = 1; ref[mid] = 1; ref[hi] = 1; }
    }
    keep[f] = k;
}

// cluster_map / kept_cluster_idx from the flags' scan (drop_unreferenced), or the identity
__global__ __launch_bounds__(kMsBlock) void ms_cluster_emit_kernel(long C, const int *__restrict__ ref, const int *__restrict__ local,
                                                                   const int *__restrict__ chunk_base, int *__restrict__ cluster_map,
                                                                   int *__restrict__ kept_cluster_idx, int *__restrict__ total) {
    const long c = (long)blockIdx.x * kMsBlock + threadIdx.x;
    if (c >= C) return;
    const int at = !ref ? (int)c : ref[c] ? ms_prefix(local, chunk_base, (int)c) : -1;
    cluster_map[c] = at;
    if (at >= 0) kept_cluster_idx[at] = (int)c;
    if (!ref && c == 0) *total = (int)C;
}

__global__ __launch_bounds__(kMsBlock) void ms_face_emit_kernel(const int *__restrict__ faces, long F, const int *__restrict__ keep, const int *__restrict__ local,
                                                                const int *__restrict__ chunk_base, const int *__restrict__ vert_cluster,
                                                                const int *__restrict__ cluster_map, int *__restrict__ faces_out, int *__restrict__ face_idx) {
    const long f = (long)blockIdx.x * kMsBlock + threadIdx.x;
    if (f >= F || !keep[f]) return;                          // (a kept face's indices and cluster ids were checked by the remap pass)
    const long at = ms_prefix(local, chunk_base, (int)f);
    faces_out[3 * at] = cluster_map[vert_cluster[faces[3 * f]]];
    faces_out[3 * at + 1] = cluster_map[vert_cluster[faces[3 * f + 1]]];
    faces_out[3 * at + 2] = cluster_map[vert_cluster[faces[3 * f + 2]]];
    face_idx[at] = (int)f;
}

__global__ __launch_bounds__(kMsBlock) void ms_vert_map_kernel(long V, const int *__restrict__ vert_cluster, long C, const int *__restrict__ cluster_map,
                                                               int *__restrict__ vert_map) {
    const long v = (long)blockIdx.x * kMsBlock + threadIdx.x;
    if (v >= V) return;
    const int c = vert_cluster[v];
    vert_map[v] = (c >= 0 && c < C) ? cluster_map[c] : -1;
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static unsigned ms_blocks(long n) { return (unsigned)((n + kMsBlock - 1) / kMsBlock); }

// exclusive scan of src[0, n) into (w.local, w.chunk_base); the sum goes to *total (device)
static void ms_scan(const MsWork &w, const int *src, long n, int *total, hipStream_t s) {
    const long nch = (n + kMsScanChunk - 1) / kMsScanChunk;
    hipLaunchKernelGGL((scan_chunks_kernel<int, int, kMsWaves>), dim3((unsigned)nch), dim3(kMsBlock), 0, s, src, n, w.local, w.chunk_tot);
    hipLaunchKernelGGL((scan_chunk_totals_kernel<int, kMsWaves>), dim3(1), dim3(kMsBlock), 0, s, (const int *)w.chunk_tot, nch, w.chunk_base, total);
}

static bool ms_sizes_ok(long V, long F) { return V >= 0 && V < (1l << 31) && F >= 0 && F <= kMsMaxFaces; }

static int ms_check_sizes(const char *what, long V, long F) {
    DFH_REQUIRE(V >= 0 && V < (1l << 31), "%s: bad vertex count %ld", what, V);
    DFH_REQUIRE(F >= 0 && F <= kMsMaxFaces, "%s: bad face count %ld", what, F);
    return DFH_OK;
}

static int ms_check_work(const char *what, long V, long F, const void *workspace, size_t workspace_bytes) {
    DFH_REQUIRE(workspace, "%s: null workspace", what);
    DFH_REQUIRE(((size_t)workspace & 7) == 0, "%s: the workspace is not 8-byte aligned", what);
    DFH_REQUIRE(workspace_bytes >= ms_carve(nullptr, nullptr, V, F), "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes,
                ms_carve(nullptr, nullptr, V, F));
    return DFH_OK;
}

static int ms_check_grid(const char *what, double cell, const double *origin) {
    DFH_REQUIRE(std::isfinite(cell) && cell > 0.0, "%s: cell must be a finite number above 0, got %g", what, cell);
    DFH_REQUIRE(origin, "%s: null origin", what);
    DFH_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), "%s: the origin is not finite", what);
    return DFH_OK;
}

}  // namespace dfh

using namespace dfh;

extern "C" size_t dfh_mesh_simplify_workspace_bytes(long n_verts, long n_faces) {
    if (!ms_sizes_ok(n_verts, n_faces)) return 0;
    return ms_carve(nullptr, nullptr, n_verts, n_faces);
}

extern "C" int dfh_mesh_simplify_keys(const void *verts, int dtype, long n_verts, const int *faces, long n_faces, double cell, const double *origin,
                                      long long *keys, void *workspace, size_t workspace_bytes, void *stream) {
    const char *what = "dfh_mesh_simplify_keys";
    const long V = n_verts, F = n_faces;
    if (int rc = ms_check_sizes(what, V, F)) return rc;
    DFH_REQUIRE(dtype == DFH_F32 || dtype == DFH_F64, "%s: bad dtype %d", what, dtype);
    if (int rc = ms_check_grid(what, cell, origin)) return rc;
    DFH_REQUIRE(V == 0 || (verts && keys), "%s: null verts or keys", what);
    DFH_REQUIRE(F == 0 || faces, "%s: null faces", what);
    if (V == 0 && F == 0) return DFH_OK;
    if (int rc = ms_check_work(what, V, F, workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    MsWork w;
    ms_carve(&w, (char *)workspace, V, F);
    const MsGrid g{cell, origin[0], origin[1], origin[2]};
    DFH_HIP_CHECK(hipMemsetAsync(w.hdr, 0, 16, s));
    if (dtype == DFH_F32)
        hipLaunchKernelGGL((ms_keys_kernel<float>), dim3(ms_blocks(V > F ? V : F)), dim3(kMsBlock), 0, s, (const float *)verts, V, faces, F, g, keys, w.hdr + 2);
    else
        hipLaunchKernelGGL((ms_keys_kernel<double>), dim3(ms_blocks(V > F ? V : F)), dim3(kMsBlock), 0, s, (const double *)verts, V, faces, F, g, keys, w.hdr + 2);
    DFH_HIP_CHECK(hipGetLastError());
    int hdr[3] = {0, 0, 0};
    DFH_HIP_CHECK(hipMemcpyAsync(hdr, w.hdr, 12, hipMemcpyDeviceToHost, s));
    DFH_HIP_CHECK(hipStreamSynchronize(s));
    DFH_REQUIRE(!(hdr[2] & kMsBadCoord), "%s: a vertex coordinate is not finite", what);
    DFH_REQUIRE(!(hdr[2] & kMsBadCell), "%s: a vertex lies outside the 2^21 cells an axis that start at the origin", what);
    DFH_REQUIRE(!(hdr[2] & kMsBadFace), "%s: a face holds a vertex index outside [0, %ld)", what, V);
    return DFH_OK;
}

extern "C" int dfh_mesh_simplify_group(const long long *sorted_keys, const long long *order, long n_verts, const int *sorted_corner_vert, long n_faces,
                                       int *vert_cluster, int *cluster_start, int *cluster_count, int *corner_begin, int *corner_end,
                                       long *n_clusters, void *workspace, size_t workspace_bytes, void *stream) {
    const char *what = "dfh_mesh_simplify_group";
    const long V = n_verts, F = n_faces;
    if (int rc = ms_check_sizes(what, V, F)) return rc;
    DFH_REQUIRE(n_clusters, "%s: null n_clusters", what);
    DFH_REQUIRE(V == 0 || (sorted_keys && order && vert_cluster && cluster_start && cluster_count && corner_begin && corner_end),
                "%s: null sorted_keys, order, vert_cluster, cluster_start, cluster_count, corner_begin or corner_end", what);
    DFH_REQUIRE(F == 0 || sorted_corner_vert, "%s: null sorted_corner_vert", what);
    DFH_REQUIRE(F == 0 || V > 0, "%s: %ld faces of no vertices", what, F);
    if (V == 0) {
        *n_clusters = 0;
        return DFH_OK;
    }
    if (int rc = ms_check_work(what, V, F, workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    MsWork w;
    ms_carve(&w, (char *)workspace, V, F);
    DFH_HIP_CHECK(hipMemsetAsync(w.hdr, 0, 16, s));
    DFH_HIP_CHECK(hipMemsetAsync(w.cnt, 0, (size_t)V * 4, s));
    DFH_HIP_CHECK(hipMemsetAsync(vert_cluster, 0xff, (size_t)V * 4, s));
    DFH_HIP_CHECK(hipMemsetAsync(corner_begin, 0, (size_t)V * 4, s));
    DFH_HIP_CHECK(hipMemsetAsync(corner_end, 0, (size_t)V * 4, s));
    hipLaunchKernelGGL(ms_heads_kernel, dim3(ms_blocks(V)), dim3(kMsBlock), 0, s, sorted_keys, order, V, w.cnt, w.hdr + 2);
    ms_scan(w, w.cnt, V, w.hdr, s);
    hipLaunchKernelGGL(ms_segments_kernel, dim3(ms_blocks(V)), dim3(kMsBlock), 0, s, sorted_keys, order, V, (const int *)w.local, (const int *)w.chunk_base,
                       vert_cluster, cluster_start, cluster_count);
    if (F > 0)
        hipLaunchKernelGGL(ms_corner_ranges_kernel, dim3(ms_blocks(3 * F)), dim3(kMsBlock), 0, s, sorted_corner_vert, 3 * F, V, corner_begin, corner_end,
                           w.hdr + 2);
    DFH_HIP_CHECK(hipGetLastError());
    int hdr[3] = {0, 0, 0};
    DFH_HIP_CHECK(hipMemcpyAsync(hdr, w.hdr, 12, hipMemcpyDeviceToHost, s));
    DFH_HIP_CHECK(hipStreamSynchronize(s));
    DFH_REQUIRE(!(hdr[2] & kMsBadOrder), "%s: order holds an entry outside [0, %ld)", what, V);
    DFH_REQUIRE(!(hdr[2] & kMsBadFace), "%s: a corner names a vertex outside [0, %ld)", what, V);
    *n_clusters = hdr[0];
    return DFH_OK;
}

template <typename VT>
static void ms_clusters_launch(const MsWork &w, const void *verts, long V, const int *faces, long F, const MsGrid &g, int mode, double reg,
                               const long long *keys, const long long *order, const long long *corner_order, const int *corner_begin,
                               const int *corner_end, const int *cluster_start, const int *cluster_count, long C, void *verts_out, int *n_fallback,
                               hipStream_t s) {
    if (mode == DFH_SIMPLIFY_QUADRIC)
        hipLaunchKernelGGL((ms_vertex_quadric_kernel<VT>), dim3(ms_blocks(V)), dim3(kMsBlock), 0, s, (const VT *)verts, V, faces, F, g, keys, corner_order,
                           corner_begin, corner_end, w.qv);
    hipLaunchKernelGGL((ms_cluster_kernel<VT>), dim3(ms_blocks(C)), dim3(kMsBlock), 0, s, (const VT *)verts, V, g, mode, reg, keys, order, cluster_start,
                       cluster_count, C, (const double *)w.qv, (VT *)verts_out, n_fallback);
}

extern "C" int dfh_mesh_simplify_clusters(const void *verts, int dtype, long n_verts, const int *faces, long n_faces, double cell, const double *origin,
                                          int mode, double reg, const long long *keys, const long long *order, const long long *corner_order,
                                          const int *corner_begin, const int *corner_end, const int *cluster_start, const int *cluster_count,
                                          long n_clusters, void *verts_out, int *n_fallback, void *workspace, size_t workspace_bytes, void *stream) {
    const char *what = "dfh_mesh_simplify_clusters";
    const long V = n_verts, F = n_faces, C = n_clusters;
    if (int rc = ms_check_sizes(what, V, F)) return rc;
    DFH_REQUIRE(dtype == DFH_F32 || dtype == DFH_F64, "%s: bad dtype %d", what, dtype);
    if (int rc = ms_check_grid(what, cell, origin)) return rc;
    DFH_REQUIRE(mode == DFH_SIMPLIFY_QUADRIC || mode == DFH_SIMPLIFY_MEAN, "%s: bad mode %d", what, mode);
    DFH_REQUIRE(std::isfinite(reg) && reg >= 0.0, "%s: reg must be a finite number that is not negative, got %g", what, reg);
    DFH_REQUIRE(C >= 0 && C <= V, "%s: %ld clusters of %ld vertices", what, C, V);
    DFH_REQUIRE(n_fallback, "%s: null n_fallback", what);
    DFH_REQUIRE(V == 0 || (verts && keys && order && corner_begin && corner_end), "%s: null verts, keys, order, corner_begin or corner_end", what);
    DFH_REQUIRE(F == 0 || (faces && corner_order), "%s: null faces or corner_order", what);
    DFH_REQUIRE(C == 0 || (cluster_start && cluster_count && verts_out), "%s: null cluster_start, cluster_count or verts_out", what);
    if (int rc = ms_check_work(what, V, F, workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    DFH_HIP_CHECK(hipMemsetAsync(n_fallback, 0, 4, s));
    if (C == 0) return DFH_OK;
    MsWork w;
    ms_carve(&w, (char *)workspace, V, F);
    const MsGrid g{cell, origin[0], origin[1], origin[2]};
    if (dtype == DFH_F32)
        ms_clusters_launch<float>(w, verts, V, faces, F, g, mode, reg, keys, order, corner_order, corner_begin, corner_end, cluster_start, cluster_count, C,
                                  verts_out, n_fallback, s);
    else
        ms_clusters_launch<double>(w, verts, V, faces, F, g, mode, reg, keys, order, corner_order, corner_begin, corner_end, cluster_start, cluster_count, C,
                                   verts_out, n_fallback, s);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

extern "C" int dfh_mesh_simplify_attr(const void *attr, int dtype, long n_verts, long width, const long long *order, const int *cluster_start,
                                      const int *cluster_count, long n_clusters, void *out, void *stream) {
    const char *what = "dfh_mesh_simplify_attr";
    const long V = n_verts, K = width, C = n_clusters;
    DFH_REQUIRE(V >= 0 && V < (1l << 31), "%s: bad vertex count %ld", what, V);
    DFH_REQUIRE(K >= 0 && K < (1l << 31), "%s: bad attribute width %ld", what, K);
    DFH_REQUIRE(dtype == DFH_F32 || dtype == DFH_F64, "%s: bad dtype %d", what, dtype);
    DFH_REQUIRE(C >= 0 && C <= V, "%s: %ld clusters of %ld vertices", what, C, V);
    if (C == 0 || K == 0) return DFH_OK;
    DFH_REQUIRE(attr && order && cluster_start && cluster_count && out, "%s: null attr, order, cluster_start, cluster_count or out", what);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == DFH_F32)
        hipLaunchKernelGGL((ms_attr_kernel<float>), dim3(ms_blocks(C * K)), dim3(kMsBlock), 0, s, (const float *)attr, V, K, order, cluster_start, cluster_count,
                           C, (float *)out);
    else
        hipLaunchKernelGGL((ms_attr_kernel<double>), dim3(ms_blocks(C * K)), dim3(kMsBlock), 0, s, (const double *)attr, V, K, order, cluster_start,
                           cluster_count, C, (double *)out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

extern "C" int dfh_mesh_simplify_faces(const int *faces, long n_verts, long n_faces, const int *vert_cluster, long n_clusters, int drop_unreferenced,
                                       int *faces_out, int *face_idx, int *cluster_map, int *kept_cluster_idx, int *vert_map, long *counts_out,
                                       void *workspace, size_t workspace_bytes, void *stream) {
    const char *what = "dfh_mesh_simplify_faces";
    const long V = n_verts, F = n_faces, C = n_clusters;
    if (int rc = ms_check_sizes(what, V, F)) return rc;
    DFH_REQUIRE(C >= 0 && C <= V, "%s: %ld clusters of %ld vertices", what, C, V);
    DFH_REQUIRE(counts_out, "%s: null counts_out", what);
    DFH_REQUIRE(drop_unreferenced == 0 || drop_unreferenced == 1, "%s: drop_unreferenced must be 0 or 1, got %d", what, drop_unreferenced);
    DFH_REQUIRE(V == 0 || (vert_cluster && vert_map), "%s: null vert_cluster or vert_map", what);
    DFH_REQUIRE(F == 0 || (faces && faces_out && face_idx), "%s: null faces, faces_out or face_idx", what);
    DFH_REQUIRE(C == 0 || (cluster_map && kept_cluster_idx), "%s: null cluster_map or kept_cluster_idx", what);
    DFH_REQUIRE(F == 0 || C > 0, "%s: %ld faces of no clusters", what, F);
    if (V == 0) {
        counts_out[0] = counts_out[1] = 0;
        return DFH_OK;
    }
    if (int rc = ms_check_work(what, V, F, workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    MsWork w;
    ms_carve(&w, (char *)workspace, V, F);
    DFH_HIP_CHECK(hipMemsetAsync(w.hdr, 0, 16, s));
    if (C > 0) {
        DFH_HIP_CHECK(hipMemsetAsync(w.ref, 0, (size_t)C * 4, s));
        if (F > 0) {
            DFH_HIP_CHECK(hipMemsetAsync(w.cnt, 0, (size_t)C * 4, s));
            DFH_HIP_CHECK(hipMemsetAsync(w.cur, 0, (size_t)C * 4, s));
            hipLaunchKernelGGL(ms_face_remap_kernel, dim3(ms_blocks(F)), dim3(kMsBlock), 0, s, faces, F, V, vert_cluster, C, w.fmin, w.fmid, w.fmax, w.cnt,
                               w.hdr + 2);
            ms_scan(w, w.cnt, C, w.hdr + 3, s);
            hipLaunchKernelGGL(ms_group_fill_kernel, dim3(ms_blocks(F)), dim3(kMsBlock), 0, s, F, (const int *)w.fmin, (const int *)w.local,
                               (const int *)w.chunk_base, w.cur, w.glist);
            hipLaunchKernelGGL(ms_face_keep_kernel, dim3(ms_blocks(F)), dim3(kMsBlock), 0, s, F, (const int *)w.fmin, (const int *)w.fmid, (const int *)w.fmax,
                               (const int *)w.cnt, (const int *)w.local, (const int *)w.chunk_base, (const int *)w.glist, w.flag, w.ref);
        }
        if (drop_unreferenced) ms_scan(w, w.ref, C, w.hdr, s);
        hipLaunchKernelGGL(ms_cluster_emit_kernel, dim3(ms_blocks(C)), dim3(kMsBlock), 0, s, C, drop_unreferenced ? (const int *)w.ref : (const int *)nullptr,
                           (const int *)w.local, (const int *)w.chunk_base, cluster_map, kept_cluster_idx, w.hdr);
        if (F > 0) {
            ms_scan(w, w.flag, F, w.hdr + 1, s);
            hipLaunchKernelGGL(ms_face_emit_kernel, dim3(ms_blocks(F)), dim3(kMsBlock), 0, s, faces, F, (const int *)w.flag, (const int *)w.local,
                               (const int *)w.chunk_base, vert_cluster, (const int *)cluster_map, faces_out, face_idx);
        }
    }
    hipLaunchKernelGGL(ms_vert_map_kernel, dim3(ms_blocks(V)), dim3(kMsBlock), 0, s, V, vert_cluster, C, (const int *)cluster_map, vert_map);
    DFH_HIP_CHECK(hipGetLastError());
    int hdr[3] = {0, 0, 0};
    DFH_HIP_CHECK(hipMemcpyAsync(hdr, w.hdr, 12, hipMemcpyDeviceToHost, s));
    DFH_HIP_CHECK(hipStreamSynchronize(s));
    DFH_REQUIRE(hdr[2] == 0, "%s: a face index outside [0, %ld) or a cluster id outside [0, %ld)", what, V, C);
    counts_out[0] = hdr[0];
    counts_out[1] = hdr[1];
    return DFH_OK;
}
