// K23  mesh connected components: label the vertices and faces of a triangle mesh by component, measure every component
// (vertices, faces, box, area) and compact the mesh to the components a caller keeps (dfh_mesh_component*, dfh_mesh_compact).
// No reference counterpart.  Every output is defined operation by operation in include/dfusion_hip.h and is a function of the
// mesh alone; tests/components_np.py restates all of it and agrees bit for bit.
//
// Labelling.  A lock-free union-find over parent[] (= the caller's root array).  Invariants, from the init kernel on:
//   (I1) parent[v] <= v;   (I2) a store to parent[v] only lowers it;   (I3) parent[v] is in v's component of the faces hooked so far.
// The three kinds of store keep them: a hook is atomicCAS(&parent[hi], hi, lo) with lo < hi, it succeeds only on a root; a
// shortening is atomicMin(&parent[x], g) with g the grandparent of x read a moment before (path halving); the flatten pass, which
// runs when no hook is in flight, stores the root it walked to (a relaxed atomic store of a value <= every ancestor of v).
// Termination of every loop in a kernel of this file:
//   cc_find      x <- parent[parent[x]] until one of the two is a root.  By (I1) x strictly decreases: at most x + 1 steps, whatever other lanes store
//                in between (a stale value is an older, larger ancestor: still < x).
//   cc_union     each pass takes the two roots found, returns if they are equal, else tries to hook hi = max under lo = min.  If
//                the CAS fails, parent[hi] = old < hi already (another lane hooked hi), hi ~ old holds, and the pass repeats with
//                (old, lo), both < hi.  max(u, v) strictly decreases from pass to pass: at most max(u, v) + 1 passes.  A lane
//                never waits for another lane's store: a failed CAS hands it a smaller pair at once.
//   cc_flatten   the walk of cc_find with no stores but the last (the hooks are over: the launch before has ended).
//   wave loops   (cc_table_verts_kernel) each turn retires at least the leader lane's component: at most 64 turns a pass, 4 passes,
//                uniform in the wave.
//   table loops  head search, head sum, rank count and the final sum run over fixed index ranges.
// The root of a tree is the lowest index of its component: by (I1) no vertex lies below its root.  Face (a, b, c) hooks (a, b)
// and (a, c); (b, c) follows by transitivity, so the closure is that of the 3F face edges.  The (a, b) of all faces go first, the
// trees are flattened, then the (a, c): by then nearly every pair hangs under one root already and costs two loads.
//
// Ids and compaction are count -> scan -> emit on dfh_scan.h's two-level pair (chunks of 1024).  Counts are integer atomics, the
// box is integer atomicMin / atomicMax on order-preserving keys, pre-reduced per wave and component (one giant component would
// otherwise send every vertex's seven atomics to the same seven words).  The area uses no float atomic: the order below.
//
// Area order.  Chunk j = the faces [256 j, 256 j + 256).  P(j, c) = the areas of chunk j's faces of component c added in
// ascending face index, starting from the first.  area[c] = the P(j, c) of the chunks that hold a face of c, added in ascending
// j, starting from the first; 0.0 for a component without faces.  On the device: one workgroup a chunk; the lowest face of each
// component in the chunk (the head) adds its component's areas from LDS and leaves one entry (j, c, P); the entries are
// grouped by component (count -> scan -> fill with an integer cursor, so in the order the atomics landed), then each entry takes
// the rank of its j among its component's entries -- the order the atomics landed in is gone -- and one wave a component adds
// the ranked partials one after the other.  The rank count is quadratic in a component's chunks (F / 256 at most: 37 M compares at 1.57 M faces).
#include <algorithm>
#include <climits>
#include <cmath>

#include "dfh_common.h"
#include "dfh_scan.h"

namespace dfh {

constexpr int kCcBlock = 256;            // threads per workgroup everywhere; also the faces of one area chunk
constexpr int kCcWaves = kCcBlock / kWave;
constexpr int kCcScanChunk = 4 * kCcBlock;
constexpr unsigned long long kCcKeyNanMin = 0ull, kCcKeyNanMax = ~0ull;
static_assert(kCcScanChunk == 1024, "ids are chunk_base[e >> 10] + local[e]");

struct CcWork {                          // the caller's workspace, cut up (N = max(V, F, 1))
    int *hdr;                            // 4 words: totals and the bad-index flag
    int *cnt, *local, *cur;              // N each
    int *chunk_tot, *chunk_base;         // N / 1024 + 1, + 2
    int *headc, *ej, *ec;                // F each
    double *tmpP, *eP;                   // F each
};

static size_t cc_align8(size_t b) { return (b + 7) & ~(size_t)7; }

static size_t cc_carve(CcWork *w, char *p, long V, long F) {
    const size_t N = (size_t)(V > F ? V : F) + 1, nch = N / kCcScanChunk + 2;
    size_t o = 0;
    auto take = [&](size_t bytes) { char *q = p ? p + o : nullptr; o += cc_align8(bytes); return q; };
    char *hdr = take(16), *cnt = take(N * 4), *local = take(N * 4), *cur = take(N * 4), *ct = take(nch * 4), *cb = take(nch * 4);
    char *headc = take((size_t)F * 4), *ej = take((size_t)F * 4), *ec = take((size_t)F * 4), *tmpP = take((size_t)F * 8), *eP = take((size_t)F * 8);
    if (w) *w = CcWork{(int *)hdr, (int *)cnt, (int *)local, (int *)cur, (int *)ct, (int *)cb, (int *)headc, (int *)ej, (int *)ec, (double *)tmpP, (double *)eP};
    return o;
}

__device__ __forceinline__ int cc_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree as far as this lane can see it; every second node on the way is handed to its grandparent (path halving)
__device__ __forceinline__ int cc_find(int *parent, int x) {
    int p = cc_load(parent + x);
    while (p != x) {
        const int g = cc_load(parent + p);
        if (g == p) return p;
        atomicMin(parent + x, g);
        x = g;
        p = cc_load(parent + x);
    }
    return x;
}

__device__ __forceinline__ void cc_union(int *parent, int u, int v) {
    for (;;) {
        u = cc_find(parent, u);
        v = cc_find(parent, v);
        if (u == v) return;
        const int hi = max(u, v), lo = min(u, v);
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        u = old;
        v = lo;
    }
}

__global__ __launch_bounds__(kCcBlock) void cc_init_kernel(int *__restrict__ parent, long V) {
    const long v = (long)blockIdx.x * kCcBlock + threadIdx.x;
    if (v < V) parent[v] = (int)v;
}

// One edge of every face: EDGE 0 = (a, b), EDGE 1 = (a, c).  Two vertices that already hang under the same node need nothing: after
// the flatten pass between the two launches that is nearly every (a, c), two loads and no atomic.
template <int EDGE>
__global__ __launch_bounds__(kCcBlock) void cc_hook_kernel(int *parent, long V, const int *__restrict__ faces, long F, int *__restrict__ bad) {
    const long f = (long)blockIdx.x * kCcBlock + threadIdx.x;
    if (f >= F) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) {
        atomicOr(bad, 1);
        return;
    }
    const int o = EDGE == 0 ? b : c;
    if (a != o && cc_load(parent + a) != cc_load(parent + o)) cc_union(parent, a, o);
}

// parent[v] = root[v]; with is_root (the last flatten of a call), is_root[v] for the scan
__global__ __launch_bounds__(kCcBlock) void cc_flatten_kernel(int *parent, long V, int *__restrict__ is_root) {
    const long v = (long)blockIdx.x * kCcBlock + threadIdx.x;
    if (v >= V) return;
    int r = (int)v, p = cc_load(parent + r);
    while (p != r) {
        r = p;
        p = cc_load(parent + r);
    }
    if (r != (int)v) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (is_root) is_root[v] = r == (int)v;
}

// component id of a root: the roots in front of it
__device__ __forceinline__ int cc_rank(const int *__restrict__ local, const int *__restrict__ chunk_base, int e) {
    return chunk_base[e >> 10] + local[e];
}

__global__ __launch_bounds__(kCcBlock) void cc_ids_kernel(const int *__restrict__ root, long V, const int *__restrict__ faces, long F,
                                                          const int *__restrict__ local, const int *__restrict__ chunk_base,
                                                          int *__restrict__ vert_comp, int *__restrict__ face_comp) {
    const long i = (long)blockIdx.x * kCcBlock + threadIdx.x;
    if (i < V) vert_comp[i] = cc_rank(local, chunk_base, root[i]);
    if (i < F) {
        const int a = faces[3 * i], b = faces[3 * i + 1], c = faces[3 * i + 2];
        const bool ok = a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V;
        face_comp[i] = ok ? cc_rank(local, chunk_base, root[a]) : -1;
    }
}

// ---- the table --------------------------------------------------------------------------------------------------------------
// order-preserving key of a double: k(x) < k(y) <=> x < y, -0.0 below +0.0; a NaN takes the key that wins its reduction
__device__ __forceinline__ unsigned long long cc_key(double x, unsigned long long nan_key) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return x != x ? nan_key : (b >> 63) ? ~b : b | (1ull << 63);
}
__device__ __forceinline__ double cc_unkey(unsigned long long k) {
    if (k == kCcKeyNanMin || k == kCcKeyNanMax) return __longlong_as_double(0x7ff8000000000000ll);
    return __longlong_as_double((long long)((k >> 63) ? k & ~(1ull << 63) : ~k));
}

__global__ __launch_bounds__(kCcBlock) void cc_table_init_kernel(long C, int *__restrict__ n_verts, int *__restrict__ n_faces,
                                                                 unsigned long long *__restrict__ kmin, unsigned long long *__restrict__ kmax,
                                                                 int *__restrict__ ecount, int *__restrict__ cursor) {
    const long c = (long)blockIdx.x * kCcBlock + threadIdx.x;
    if (c >= C) return;
    n_verts[c] = 0; n_faces[c] = 0; ecount[c] = 0; cursor[c] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { kmin[3 * c + a] = ~0ull; kmax[3 * c + a] = 0ull; }
}

__device__ __forceinline__ unsigned long long cc_wave_min(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const unsigned long long y = __shfl_xor(v, m, kWave); v = y < v ? y : v; }
    return v;
}
__device__ __forceinline__ unsigned long long cc_wave_max(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const unsigned long long y = __shfl_xor(v, m, kWave); v = y > v ? y : v; }
    return v;
}

// One wave walks kCcVertPasses * 64 consecutive vertices.  Per pass it reduces per component (the loop retires the leader lane's
// component each time round); what it has reduced stays in registers while the next piece belongs to the same component, so a
// component that owns a long run of vertices is sent to the table once a wave, not once a lane.
constexpr int kCcVertPasses = 4;

__device__ __forceinline__ void cc_table_flush(int lane, int c, int n, const unsigned long long (&lo)[3], const unsigned long long (&hi)[3],
                                               int *__restrict__ n_verts, unsigned long long *__restrict__ kmin, unsigned long long *__restrict__ kmax) {
    if (c < 0 || lane != 0) return;
    atomicAdd(n_verts + c, n);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicMin(kmin + 3 * (long)c + a, lo[a]);
        atomicMax(kmax + 3 * (long)c + a, hi[a]);
    }
}

template <typename VT>
__global__ __launch_bounds__(kCcBlock) void cc_table_verts_kernel(const VT *__restrict__ verts, long V, const int *__restrict__ root,
                                                                  const int *__restrict__ vert_comp, long C, int *__restrict__ comp_root,
                                                                  int *__restrict__ n_verts, unsigned long long *__restrict__ kmin,
                                                                  unsigned long long *__restrict__ kmax) {
    const int lane = threadIdx.x & 63;
    const long wave = ((long)blockIdx.x * kCcBlock + threadIdx.x) >> 6;
    int acc_c = -1, acc_n = 0;                               // (the same in every lane)
    unsigned long long acc_lo[3] = {~0ull, ~0ull, ~0ull}, acc_hi[3] = {0ull, 0ull, 0ull};
    for (int pass = 0; pass < kCcVertPasses; ++pass) {
        const long v0 = (wave * kCcVertPasses + pass) * kWave;
        if (v0 >= V) break;
        const long v = v0 + lane;
        int c = v < V ? vert_comp[v] : -1;
        if (c < 0 || c >= C) c = -1;
        unsigned long long lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = c >= 0 ? (double)verts[3 * v + a] : 0.0;
            lo[a] = cc_key(x, kCcKeyNanMin);
            hi[a] = cc_key(x, kCcKeyNanMax);
        }
        if (c >= 0 && root[v] == (int)v) comp_root[c] = (int)v;
        bool todo = c >= 0;
        for (;;) {
            const unsigned long long left = __ballot(todo);
            if (!left) break;
            const int leader = __ffsll((long long)left) - 1;
            const int lc = __shfl(c, leader, kWave);
            const bool mine = todo && c == lc;
            const int n = __popcll(__ballot(mine));
            if (lc != acc_c) {
                cc_table_flush(lane, acc_c, acc_n, acc_lo, acc_hi, n_verts, kmin, kmax);
                acc_c = lc;
                acc_n = 0;
#pragma unroll
                for (int a = 0; a < 3; ++a) { acc_lo[a] = ~0ull; acc_hi[a] = 0ull; }
            }
            acc_n += n;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const unsigned long long l = cc_wave_min(mine ? lo[a] : ~0ull), h = cc_wave_max(mine ? hi[a] : 0ull);
                acc_lo[a] = l < acc_lo[a] ? l : acc_lo[a];
                acc_hi[a] = h > acc_hi[a] ? h : acc_hi[a];
            }
            if (mine) todo = false;
        }
    }
    cc_table_flush(lane, acc_c, acc_n, acc_lo, acc_hi, n_verts, kmin, kmax);
}

// one workgroup a chunk of 256 faces: areas, the heads' partial sums, the entry and face counts
template <typename VT>
__global__ __launch_bounds__(kCcBlock) void cc_table_faces_kernel(const VT *__restrict__ verts, long V, const int *__restrict__ faces, long F,
                                                                  const int *__restrict__ face_comp, long C, int *__restrict__ n_faces,
                                                                  int *__restrict__ ecount, int *__restrict__ headc, double *__restrict__ tmpP) {
    __shared__ int sc[kCcBlock];
    __shared__ double sa[kCcBlock];
    const int t = threadIdx.x;
    const long f = (long)blockIdx.x * kCcBlock + t;
    int c = f < F ? face_comp[f] : -1;
    double area = 0.0;
    if (c >= 0 && c < C) {
        const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
        if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) c = -1;
        else {
            const double ax = (double)verts[3 * (long)ia], ay = (double)verts[3 * (long)ia + 1], az = (double)verts[3 * (long)ia + 2];
            const double e1x = (double)verts[3 * (long)ib] - ax, e1y = (double)verts[3 * (long)ib + 1] - ay, e1z = (double)verts[3 * (long)ib + 2] - az;
            const double e2x = (double)verts[3 * (long)ic] - ax, e2y = (double)verts[3 * (long)ic + 1] - ay, e2z = (double)verts[3 * (long)ic + 2] - az;
            const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
            area = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
        }
    } else c = -1;
    sc[t] = c;
    sa[t] = area;
    __syncthreads();
    bool head = c >= 0;
    for (int i = t - 1; head && i >= 0; --i) head = sc[i] != c;
    if (f < F) headc[f] = head ? c : -1;
    if (!head) return;
    double s = area;
    int members = 1;
    for (int i = t + 1; i < kCcBlock; ++i)
        if (sc[i] == c) { s += sa[i]; ++members; }
    tmpP[f] = s;
    atomicAdd(ecount + c, 1);
    atomicAdd(n_faces + c, members);
}

__global__ __launch_bounds__(kCcBlock) void cc_table_fill_kernel(long F, const int *__restrict__ headc, const double *__restrict__ tmpP,
                                                                 const int *__restrict__ local, const int *__restrict__ chunk_base,
                                                                 int *__restrict__ cursor, int *__restrict__ ej, int *__restrict__ ec, double *__restrict__ eP) {
    const long f = (long)blockIdx.x * kCcBlock + threadIdx.x;
    if (f >= F) return;
    const int c = headc[f];
    if (c < 0) return;
    const long pos = (long)cc_rank(local, chunk_base, c) + atomicAdd(cursor + c, 1);
    if (pos >= F) return;                                    // (cannot happen: the entries are at most the faces)
    ej[pos] = (int)(f >> 8);
    ec[pos] = c;
    eP[pos] = tmpP[f];
}

// one wave an entry at a time: it goes to the rank of its chunk among its component's entries (the lanes share the count).  The
// grid is bounded (the entries are known on the device only): a wave strides over the entries, a fixed range.
constexpr int kCcRankBlocks = 2048;

__global__ __launch_bounds__(kCcBlock) void cc_table_rank_kernel(long F, const int *__restrict__ n_entries, const int *__restrict__ ecount,
                                                                 const int *__restrict__ local, const int *__restrict__ chunk_base,
                                                                 const int *__restrict__ ej, const int *__restrict__ ec, const double *__restrict__ eP,
                                                                 double *__restrict__ sorted) {
    const int lane = threadIdx.x & 63;
    const long n_waves = (long)gridDim.x * kCcWaves;
    const long E = *n_entries < F ? *n_entries : F;
    for (long pos = (long)blockIdx.x * kCcWaves + (threadIdx.x >> 6); pos < E; pos += n_waves) {
        const int c = ec[pos], j = ej[pos];
        const long s = cc_rank(local, chunk_base, c);
        const int n = ecount[c];
        int rank = 0;
        for (int i = lane; i < n && s + i < F; i += kWave) rank += ej[s + i] < j;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) rank += __shfl_xor(rank, m, kWave);
        if (lane == 0) sorted[s + rank] = eP[pos];
    }
}

// one wave a component: the box back from its keys, and the ranked partials added one after the other (the lanes load 64 at a
// time, the additions stay in their order)
__global__ __launch_bounds__(kCcBlock) void cc_table_final_kernel(long C, bool has_faces, const int *__restrict__ ecount, const int *__restrict__ local,
                                                                  const int *__restrict__ chunk_base, const double *__restrict__ sorted, long F,
                                                                  unsigned long long *kmin, unsigned long long *kmax, double *__restrict__ area) {
    const int lane = threadIdx.x & 63;
    const long c = ((long)blockIdx.x * kCcBlock + threadIdx.x) >> 6;
    if (c >= C) return;
    if (lane < 3) {
        ((double *)kmin)[3 * c + lane] = cc_unkey(kmin[3 * c + lane]);
        ((double *)kmax)[3 * c + lane] = cc_unkey(kmax[3 * c + lane]);
    }
    double s = 0.0;
    const int n = has_faces ? ecount[c] : 0;
    if (n > 0) {
        const long at = cc_rank(local, chunk_base, (int)c);
        for (int base = 0; base < n; base += kWave) {
            const double mine = (base + lane < n && at + base + lane < F) ? sorted[at + base + lane] : 0.0;
            const int m = min(kWave, n - base);
            for (int i = 0; i < m; ++i) {
                const double t = __shfl(mine, i, kWave);
                s = (base == 0 && i == 0) ? t : s + t;
            }
        }
    }
    if (lane == 0) area[c] = s;
}

// ---- compaction -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool cc_face_kept(const int *__restrict__ faces, long f, long V, const int *__restrict__ face_comp, long C,
                                             const unsigned char *__restrict__ keep, int *__restrict__ bad, int &a, int &b, int &c) {
    a = faces[3 * f]; b = faces[3 * f + 1]; c = faces[3 * f + 2];
    const int k = face_comp[f];
    if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V || k < 0 || k >= C) {
        atomicOr(bad, 1);
        return false;
    }
    return keep[k] != 0;
}

__global__ __launch_bounds__(kCcBlock) void cc_mark_kernel(const int *__restrict__ faces, long F, long V, const int *__restrict__ face_comp, long C,
                                                           const unsigned char *__restrict__ keep, int *__restrict__ ref, int *__restrict__ bad) {
    const long f = (long)blockIdx.x * kCcBlock + threadIdx.x;
    if (f >= F) return;
    int a, b, c;
    if (!cc_face_kept(faces, f, V, face_comp, C, keep, bad, a, b, c)) return;
    ref[a] = 1; ref[b] = 1; ref[c] = 1;
}

__global__ __launch_bounds__(kCcBlock) void cc_vert_flag_kernel(long V, const int *__restrict__ vert_comp, long C, const unsigned char *__restrict__ keep,
                                                                int *__restrict__ flag, int *__restrict__ bad) {
    const long v = (long)blockIdx.x * kCcBlock + threadIdx.x;
    if (v >= V) return;
    const int k = vert_comp[v];
    if (k < 0 || k >= C) {
        atomicOr(bad, 1);
        flag[v] = 0;
        return;
    }
    flag[v] = keep[k] != 0;
}

__global__ __launch_bounds__(kCcBlock) void cc_vert_emit_kernel(long V, const int *__restrict__ flag, const int *__restrict__ local,
                                                                const int *__restrict__ chunk_base, int *__restrict__ vert_map,
                                                                int *__restrict__ kept_vert_idx) {
    const long v = (long)blockIdx.x * kCcBlock + threadIdx.x;
    if (v >= V) return;
    const int at = flag[v] ? cc_rank(local, chunk_base, (int)v) : -1;
    vert_map[v] = at;
    if (at >= 0) kept_vert_idx[at] = (int)v;
}

__global__ __launch_bounds__(kCcBlock) void cc_face_flag_kernel(const int *__restrict__ faces, long F, long V, const int *__restrict__ face_comp, long C,
                                                                const unsigned char *__restrict__ keep, int *__restrict__ flag, int *__restrict__ bad) {
    const long f = (long)blockIdx.x * kCcBlock + threadIdx.x;
    if (f >= F) return;
    int a, b, c;
    flag[f] = cc_face_kept(faces, f, V, face_comp, C, keep, bad, a, b, c);
}

__global__ __launch_bounds__(kCcBlock) void cc_face_emit_kernel(const int *__restrict__ faces, long F, const int *__restrict__ flag,
                                                                const int *__restrict__ local, const int *__restrict__ chunk_base,
                                                                const int *__restrict__ vert_map, int *__restrict__ faces_out) {
    const long f = (long)blockIdx.x * kCcBlock + threadIdx.x;
    if (f >= F || !flag[f]) return;                          // (a kept face's indices were checked by the flag pass)
    const long at = cc_rank(local, chunk_base, (int)f);
    faces_out[3 * at] = vert_map[faces[3 * f]];
    faces_out[3 * at + 1] = vert_map[faces[3 * f + 1]];
    faces_out[3 * at + 2] = vert_map[faces[3 * f + 2]];
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static unsigned cc_blocks(long n) { return (unsigned)((n + kCcBlock - 1) / kCcBlock); }

// exclusive scan of w.cnt[0, n) into (w.local, w.chunk_base); the sum goes to *total (device)
static void cc_scan(const CcWork &w, long n, int *total, hipStream_t s) {
    const long nch = (n + kCcScanChunk - 1) / kCcScanChunk;
    hipLaunchKernelGGL((scan_chunks_kernel<int, int, kCcWaves>), dim3((unsigned)nch), dim3(kCcBlock), 0, s, (const int *)w.cnt, n, w.local, w.chunk_tot);
    hipLaunchKernelGGL((scan_chunk_totals_kernel<int, kCcWaves>), dim3(1), dim3(kCcBlock), 0, s, (const int *)w.chunk_tot, nch, w.chunk_base, total);
}

static int cc_check_sizes(const char *what, long V, long F) {
    DFH_REQUIRE(V >= 0 && V < (1l << 31), "%s: bad vertex count %ld", what, V);
    DFH_REQUIRE(F >= 0 && F < (1l << 31), "%s: bad face count %ld", what, F);
    return DFH_OK;
}

static int cc_check_work(const char *what, long V, long F, const void *workspace, size_t workspace_bytes) {
    DFH_REQUIRE(workspace, "%s: null workspace", what);
    DFH_REQUIRE(((size_t)workspace & 7) == 0, "%s: the workspace is not 8-byte aligned", what);
    DFH_REQUIRE(workspace_bytes >= cc_carve(nullptr, nullptr, V, F), "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes,
                cc_carve(nullptr, nullptr, V, F));
    return DFH_OK;
}

}  // namespace dfh

using namespace dfh;

extern "C" size_t dfh_mesh_components_workspace_bytes(long n_verts, long n_faces) {
    if (n_verts < 0 || n_verts >= (1l << 31) || n_faces < 0 || n_faces >= (1l << 31)) return 0;
    return cc_carve(nullptr, nullptr, n_verts, n_faces);
}

extern "C" int dfh_mesh_components(const int *faces, long n_verts, long n_faces, int *root, int *vert_comp, int *face_comp,
                                   long *n_components, void *workspace, size_t workspace_bytes, void *stream) {
    const char *what = "dfh_mesh_components";
    const long V = n_verts, F = n_faces;
    if (int rc = cc_check_sizes(what, V, F)) return rc;
    DFH_REQUIRE(n_components, "%s: null n_components", what);
    DFH_REQUIRE(V == 0 || (root && vert_comp), "%s: null root or vert_comp", what);
    DFH_REQUIRE(F == 0 || (faces && face_comp), "%s: null faces or face_comp", what);
    if (V == 0 && F == 0) {
        *n_components = 0;
        return DFH_OK;
    }
    if (int rc = cc_check_work(what, V, F, workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    CcWork w;
    cc_carve(&w, (char *)workspace, V, F);
    DFH_HIP_CHECK(hipMemsetAsync(w.hdr, 0, 16, s));
    if (V > 0) hipLaunchKernelGGL(cc_init_kernel, dim3(cc_blocks(V)), dim3(kCcBlock), 0, s, root, V);
    if (F > 0) {
        hipLaunchKernelGGL(cc_hook_kernel<0>, dim3(cc_blocks(F)), dim3(kCcBlock), 0, s, root, V, faces, F, w.hdr + 1);
        if (V > 0) hipLaunchKernelGGL(cc_flatten_kernel, dim3(cc_blocks(V)), dim3(kCcBlock), 0, s, root, V, (int *)nullptr);
        hipLaunchKernelGGL(cc_hook_kernel<1>, dim3(cc_blocks(F)), dim3(kCcBlock), 0, s, root, V, faces, F, w.hdr + 1);
    }
    if (V > 0) {
        hipLaunchKernelGGL(cc_flatten_kernel, dim3(cc_blocks(V)), dim3(kCcBlock), 0, s, root, V, w.cnt);
        cc_scan(w, V, w.hdr, s);
    }
    hipLaunchKernelGGL(cc_ids_kernel, dim3(cc_blocks(V > F ? V : F)), dim3(kCcBlock), 0, s, (const int *)root, V, faces, F, (const int *)w.local,
                       (const int *)w.chunk_base, vert_comp, face_comp);
    DFH_HIP_CHECK(hipGetLastError());
    int hdr[2] = {0, 0};
    DFH_HIP_CHECK(hipMemcpyAsync(hdr, w.hdr, 8, hipMemcpyDeviceToHost, s));
    DFH_HIP_CHECK(hipStreamSynchronize(s));
    *n_components = hdr[0];
    DFH_REQUIRE(hdr[1] == 0, "%s: a face holds a vertex index outside [0, %ld)", what, V);
    return DFH_OK;
}

template <typename VT>
static void cc_table_launch(const CcWork &w, const void *verts, long V, const int *faces, long F, const int *root, const int *vert_comp,
                            const int *face_comp, long C, int *comp_root, int *n_verts, int *n_faces, double *bbox_min, double *bbox_max,
                            double *area, hipStream_t s) {
    unsigned long long *kmin = (unsigned long long *)bbox_min, *kmax = (unsigned long long *)bbox_max;
    hipLaunchKernelGGL(cc_table_init_kernel, dim3(cc_blocks(C)), dim3(kCcBlock), 0, s, C, n_verts, n_faces, kmin, kmax, w.cnt, w.cur);
    hipLaunchKernelGGL((cc_table_verts_kernel<VT>), dim3(cc_blocks((V + kCcVertPasses - 1) / kCcVertPasses)), dim3(kCcBlock), 0, s, (const VT *)verts, V, root, vert_comp, C, comp_root,
                       n_verts, kmin, kmax);
    if (F > 0) {
        hipLaunchKernelGGL((cc_table_faces_kernel<VT>), dim3(cc_blocks(F)), dim3(kCcBlock), 0, s, (const VT *)verts, V, faces, F, face_comp, C, n_faces,
                           w.cnt, w.headc, w.tmpP);
        cc_scan(w, C, w.hdr, s);
        hipLaunchKernelGGL(cc_table_fill_kernel, dim3(cc_blocks(F)), dim3(kCcBlock), 0, s, F, (const int *)w.headc, (const double *)w.tmpP,
                           (const int *)w.local, (const int *)w.chunk_base, w.cur, w.ej, w.ec, w.eP);
        hipLaunchKernelGGL(cc_table_rank_kernel, dim3(std::min<unsigned>(cc_blocks(F * kWave), kCcRankBlocks)), dim3(kCcBlock), 0, s, F, (const int *)w.hdr, (const int *)w.cnt,
                           (const int *)w.local, (const int *)w.chunk_base, (const int *)w.ej, (const int *)w.ec, (const double *)w.eP, w.tmpP);
    }
    hipLaunchKernelGGL(cc_table_final_kernel, dim3(cc_blocks(C * kWave)), dim3(kCcBlock), 0, s, C, F > 0, (const int *)w.cnt, (const int *)w.local,
                       (const int *)w.chunk_base, (const double *)w.tmpP, F, kmin, kmax, area);
}

extern "C" int dfh_mesh_component_table(const void *verts, int dtype, long n_verts, const int *faces, long n_faces, const int *root,
                                        const int *vert_comp, const int *face_comp, long n_components, int *comp_root, int *comp_n_verts,
                                        int *comp_n_faces, double *bbox_min, double *bbox_max, double *area, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    const char *what = "dfh_mesh_component_table";
    const long V = n_verts, F = n_faces, C = n_components;
    if (int rc = cc_check_sizes(what, V, F)) return rc;
    DFH_REQUIRE(dtype == DFH_F32 || dtype == DFH_F64, "%s: bad dtype %d", what, dtype);
    DFH_REQUIRE(C >= 0 && C <= V, "%s: %ld components of %ld vertices", what, C, V);
    DFH_REQUIRE(V == 0 || (verts && root && vert_comp), "%s: null verts, root or vert_comp", what);
    DFH_REQUIRE(F == 0 || (faces && face_comp), "%s: null faces or face_comp", what);
    DFH_REQUIRE(C == 0 || (comp_root && comp_n_verts && comp_n_faces && bbox_min && bbox_max && area), "%s: null table array", what);
    if (C == 0) return DFH_OK;
    if (int rc = cc_check_work(what, V, F, workspace, workspace_bytes)) return rc;
    CcWork w;
    cc_carve(&w, (char *)workspace, V, F);
    if (dtype == DFH_F32)
        cc_table_launch<float>(w, verts, V, faces, F, root, vert_comp, face_comp, C, comp_root, comp_n_verts, comp_n_faces, bbox_min, bbox_max, area,
                               (hipStream_t)stream);
    else
        cc_table_launch<double>(w, verts, V, faces, F, root, vert_comp, face_comp, C, comp_root, comp_n_verts, comp_n_faces, bbox_min, bbox_max, area,
                                (hipStream_t)stream);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

extern "C" int dfh_mesh_compact(const int *faces, long n_verts, long n_faces, const int *vert_comp, const int *face_comp,
                                const unsigned char *keep, long n_components, int drop_unreferenced, int *kept_vert_idx, int *vert_map,
                                int *faces_out, long *counts_out, void *workspace, size_t workspace_bytes, void *stream) {
    const char *what = "dfh_mesh_compact";
    const long V = n_verts, F = n_faces, C = n_components;
    if (int rc = cc_check_sizes(what, V, F)) return rc;
    DFH_REQUIRE(C >= 0 && C <= V, "%s: %ld components of %ld vertices", what, C, V);
    DFH_REQUIRE(counts_out, "%s: null counts_out", what);
    DFH_REQUIRE(C == 0 || keep, "%s: null keep", what);
    DFH_REQUIRE(V == 0 || (vert_comp && kept_vert_idx && vert_map), "%s: null vert_comp, kept_vert_idx or vert_map", what);
    DFH_REQUIRE(F == 0 || (faces && face_comp && faces_out), "%s: null faces, face_comp or faces_out", what);
    DFH_REQUIRE(drop_unreferenced == 0 || drop_unreferenced == 1, "%s: drop_unreferenced must be 0 or 1, got %d", what, drop_unreferenced);
    if (V == 0 && F == 0) {
        counts_out[0] = counts_out[1] = 0;
        return DFH_OK;
    }
    if (int rc = cc_check_work(what, V, F, workspace, workspace_bytes)) return rc;
    counts_out[0] = counts_out[1] = 0;
    hipStream_t s = (hipStream_t)stream;
    CcWork w;
    cc_carve(&w, (char *)workspace, V, F);
    DFH_HIP_CHECK(hipMemsetAsync(w.hdr, 0, 16, s));
    if (V > 0) {
        if (drop_unreferenced) {
            DFH_HIP_CHECK(hipMemsetAsync(w.cnt, 0, (size_t)V * 4, s));
            if (F > 0) hipLaunchKernelGGL(cc_mark_kernel, dim3(cc_blocks(F)), dim3(kCcBlock), 0, s, faces, F, V, face_comp, C, keep, w.cnt, w.hdr + 2);
        } else {
            hipLaunchKernelGGL(cc_vert_flag_kernel, dim3(cc_blocks(V)), dim3(kCcBlock), 0, s, V, vert_comp, C, keep, w.cnt, w.hdr + 2);
        }
        cc_scan(w, V, w.hdr, s);
        hipLaunchKernelGGL(cc_vert_emit_kernel, dim3(cc_blocks(V)), dim3(kCcBlock), 0, s, V, (const int *)w.cnt, (const int *)w.local,
                           (const int *)w.chunk_base, vert_map, kept_vert_idx);
    }
    if (F > 0) {
        hipLaunchKernelGGL(cc_face_flag_kernel, dim3(cc_blocks(F)), dim3(kCcBlock), 0, s, faces, F, V, face_comp, C, keep, w.cnt, w.hdr + 2);
        cc_scan(w, F, w.hdr + 1, s);
        hipLaunchKernelGGL(cc_face_emit_kernel, dim3(cc_blocks(F)), dim3(kCcBlock), 0, s, faces, F, (const int *)w.cnt, (const int *)w.local,
                           (const int *)w.chunk_base, (const int *)vert_map, faces_out);
    }
    DFH_HIP_CHECK(hipGetLastError());
    int hdr[3] = {0, 0, 0};
    DFH_HIP_CHECK(hipMemcpyAsync(hdr, w.hdr, 12, hipMemcpyDeviceToHost, s));
    DFH_HIP_CHECK(hipStreamSynchronize(s));
    DFH_REQUIRE(hdr[2] == 0, "%s: a face index outside [0, %ld) or a component id outside [0, %ld)", what, V, C);
    counts_out[0] = hdr[0];
    counts_out[1] = hdr[1];
    return DFH_OK;
}
