// K15  per-pixel features pooled onto vertices: dfh_pool_features (definition: include/dfusion_hip.h), the ordered segmented
// float32 mean of the reference's compute_correspondence (core/sdf.py:138-149), where it is a Python loop over the pixels.
//
// A float32 sum depends on its order, so the pixels of a vertex are summed in ascending pixel index, whatever the schedule.
// Launch sequence, no host synchronisation, no floating-point atomic:
//   pool_count_kernel      one lane per pixel: slot[p] = cnt[v]++ (integer atomic; the COUNT does not depend on the order, the
//                          slots of a vertex's pixels are 0 .. cnt[v] - 1 in the order the schedule chose)
//   scan_chunks_kernel     (dfh_scan.h) a workgroup scans kPoolScanChunk counts from zero and leaves the chunk's total
//   scan_chunk_totals_kernel  (dfh_scan.h) ONE workgroup scans the chunk totals: vertex v's segment starts at
//                          chunk_base[v / chunk] + local[v]
//   pool_scatter_kernel    one lane per pixel: its index goes to its slot of its vertex's segment (no second atomic) -- the
//                          segment now holds the right SET of pixels in an order the schedule chose
//   pool_order_kernel      one wave per vertex: a segment of up to kPoolCap entries is ordered in LDS by counting, for every
//                          entry, the entries below it (pixel indices are distinct, so the ranks are a permutation); a longer
//                          segment's vertex goes onto a list
//   pool_order_big_kernel  a fixed grid pulls the listed vertices; a workgroup finds the segment's smallest and largest pixel,
//                          walks vid[] over that range in order and writes the matching indices as it meets them (an ordered
//                          compaction through dfh_scan.h's block_scan_exclusive: correct for any length, one vertex may own
//                          every pixel)
//   pool_sum_kernel        `dim` lanes per vertex, lane c owns channel c: every 4 * dim-byte feature row is read by one group
//                          of adjacent lanes, the additions of a channel are one lane's chain
#include <cstdint>

#include "dfh_common.h"
#include "dfh_scan.h"

namespace dfh {

constexpr int kPoolBlock = 256;
constexpr int kPoolScanChunk = 1024;  // counts per workgroup of the scan (256 lanes x 4)
// Segment entries one wave orders in LDS: 4 KiB a wave, 16 KiB a workgroup, so the eight workgroups a CU's wave slots admit
// fit its LDS.  The ordering costs n^2 / 64 LDS words read per lane (as 16-byte broadcasts): 4 k at the cap, a few at the
// tens to hundreds of pixels a vertex of a body mesh collects over 24 views.
constexpr int kPoolCap = 1024;
constexpr int kPoolWaves = kPoolBlock / kWave;   // vertices per workgroup of the ordering pass
constexpr int kPoolBigStep = 4 * kPoolBlock;     // pixels per step of the long-segment walk

struct PoolLayout {
    size_t local, chunk_tot, chunk_base, big_n, big, slot, list, end;
    long nchunks, big_cap;
};

static PoolLayout pool_layout(long n_pixels, long n_verts) {
    PoolLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 15) / 16 * 16; return at; };
    L.nchunks = (n_verts + kPoolScanChunk - 1) / kPoolScanChunk;
    L.big_cap = n_pixels / (kPoolCap + 1) + 1;       // more vertices than that cannot own more than kPoolCap pixels each
    L.local = take(4 * (size_t)n_verts);
    L.chunk_tot = take(4 * (size_t)L.nchunks);
    L.chunk_base = take(4 * (size_t)L.nchunks);
    L.big_n = take(4);
    L.big = take(4 * (size_t)L.big_cap);
    L.slot = take(4 * (size_t)n_pixels);             // written and read for the pixels with a vertex only
    L.list = take(4 * (size_t)n_pixels);
    L.end = o;
    return L;
}

struct PoolSegs {                     // where vertex v's segment starts
    const int *local, *chunk_base;
    __device__ __forceinline__ int start(long v) const { return chunk_base[v / kPoolScanChunk] + local[v]; }
};

__global__ __launch_bounds__(kPoolBlock) void pool_count_kernel(const int *__restrict__ vid, long n_pixels, long n_verts,
                                                                int *__restrict__ cnt, int *__restrict__ slot) {
    const long p = (long)blockIdx.x * kPoolBlock + threadIdx.x;
    if (p >= n_pixels) return;
    const int v = vid[p];
    if (v >= 0 && v < n_verts) slot[p] = atomicAdd(cnt + v, 1);
}

// The segment starts: dfh_scan.h's two-level pair.  local[v] = pixels of the vertices of v's chunk in front of v, chunk_tot[chunk] =
// pixels of the chunk, chunk_base[c] = pixels in front of chunk c (all < 2^31: n_pixels is)
static_assert(kPoolScanChunk == 4 * kPoolBlock, "scan_chunks_kernel takes four counts a thread");

__global__ __launch_bounds__(kPoolBlock) void pool_scatter_kernel(const int *__restrict__ vid, long n_pixels, long n_verts, PoolSegs segs,
                                                                  const int *__restrict__ slot, int *__restrict__ list) {
    const long p = (long)blockIdx.x * kPoolBlock + threadIdx.x;
    if (p >= n_pixels) return;
    const int v = vid[p];
    if (v < 0 || v >= n_verts) return;
    list[segs.start(v) + slot[p]] = (int)p;              // slot < cnt[v]: the count pass wrote it for this very id
}

// One wave per vertex.  The barriers stand at workgroup-uniform places, outside the per-wave loops.
__global__ __launch_bounds__(kPoolBlock) void pool_order_kernel(long n_verts, const int *__restrict__ cnt, PoolSegs segs,
                                                                int *__restrict__ list, int *__restrict__ big_n, int *__restrict__ big) {
    __shared__ __attribute__((aligned(16))) int seg[kPoolWaves][kPoolCap];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long v = (long)blockIdx.x * kPoolWaves + wv;
    int n = v < n_verts ? cnt[v] : 0;
    int s = 0;
    if (n > kPoolCap) {
        if (lane == 0) big[atomicAdd(big_n, 1)] = (int)v;  // capacity n_pixels / (cap + 1) + 1: never overflows
        n = 0;
    }
    if (n > 1) {
        s = segs.start(v);
        const int n4 = (n + 3) & ~3;                     // padded with INT_MAX: never below an entry
        for (int i = lane; i < n4; i += kWave) seg[wv][i] = i < n ? list[s + i] : 0x7fffffff;
    }
    __syncthreads();
    if (n > 1) {
        const int4 *row = reinterpret_cast<const int4 *>(seg[wv]);
        const int n4 = (n + 3) >> 2;
        for (int i = lane; i < n; i += kWave) {
            const int mine = seg[wv][i];
            int rank = 0;
            for (int j = 0; j < n4; ++j) {               // (the same address in every lane: a broadcast)
                const int4 o = row[j];
                rank += (o.x < mine) + (o.y < mine) + (o.z < mine) + (o.w < mine);
            }
            list[s + rank] = mine;                       // the segment is in LDS: nothing reads list[s ..] any more
        }
    }
}

__global__ __launch_bounds__(kPoolBlock) void pool_order_big_kernel(const int *__restrict__ vid, const int *__restrict__ cnt, PoolSegs segs,
                                                                    int *__restrict__ list, const int *__restrict__ big_n,
                                                                    const int *__restrict__ big) {
    __shared__ int red_lo[kPoolWaves], red_hi[kPoolWaves], wcnt[kPoolWaves];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int nbig = *big_n;
    for (int e = blockIdx.x; e < nbig; e += gridDim.x) {
        const int v = big[e];
        const int n = cnt[v], s = segs.start(v);
        int lo = 0x7fffffff, hi = -1;
        for (int i = t; i < n; i += kPoolBlock) {
            const int p = list[s + i];
            lo = p < lo ? p : lo;
            hi = p > hi ? p : hi;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
            lo = a < lo ? a : lo;
            hi = b > hi ? b : hi;
        }
        if (lane == 0) { red_lo[wv] = lo; red_hi[wv] = hi; }
        __syncthreads();                                 // every read of the unordered segment is done
#pragma unroll
        for (int w_ = 0; w_ < kPoolWaves; ++w_) {
            lo = red_lo[w_] < lo ? red_lo[w_] : lo;
            hi = red_hi[w_] > hi ? red_hi[w_] : hi;
        }
        int run = 0;                                     // entries written so far
        for (long b0 = lo; b0 <= hi; b0 += kPoolBigStep) {
            const long p0 = b0 + 4 * (long)t;            // lane t takes pixels p0 .. p0 + 3: lane order is pixel order
            bool m[4];
            int c = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m[j] = p0 + j <= hi && vid[p0 + j] == v;
                c += m[j];
            }
            int all;
            const int off = block_scan_exclusive<kPoolWaves>(c, wcnt, all);
            int at = s + run + off;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (m[j]) list[at++] = (int)(p0 + j);
            run += all;
            __syncthreads();                             // wcnt is rewritten by the next step
        }
        __syncthreads();                                 // red_lo / red_hi are rewritten by the next vertex
    }
}

// dim lanes per vertex; a workgroup takes kPoolBlock / dim vertices (its last kPoolBlock % dim lanes idle).
__global__ __launch_bounds__(kPoolBlock) void pool_sum_kernel(const float *__restrict__ feat, int dim, long n_verts, const int *__restrict__ cnt,
                                                              PoolSegs segs, const int *__restrict__ list, float *__restrict__ out) {
    const int per = kPoolBlock / dim;
    const int g = threadIdx.x / dim, c = threadIdx.x - g * dim;
    const long v = (long)blockIdx.x * per + g;
    if (g >= per || v >= n_verts) return;
    const int n = cnt[v];
    float acc = 0.0f;
    if (n > 0) {
        const int *seg = list + segs.start(v);
        int i = 0;
        for (; i + 4 <= n; i += 4) {                     // four rows in flight, added in order
            const float f0 = feat[(size_t)seg[i] * dim + c], f1 = feat[(size_t)seg[i + 1] * dim + c];
            const float f2 = feat[(size_t)seg[i + 2] * dim + c], f3 = feat[(size_t)seg[i + 3] * dim + c];
            acc = acc + f0;
            acc = acc + f1;
            acc = acc + f2;
            acc = acc + f3;
        }
        for (; i < n; ++i) acc = acc + feat[(size_t)seg[i] * dim + c];
        acc = acc / (float)n;
    }
    out[(size_t)v * dim + c] = acc;
}

static const char *pool_check_sizes(long n_pixels, int dim, long n_verts) {
    if (dim < 1 || dim > 64) return "dim outside 1..64";
    if (n_pixels < 0 || n_pixels >= (1L << 31)) return "n_pixels outside [0, 2^31)";
    if (n_verts < 0 || n_verts >= (1L << 31)) return "n_verts outside [0, 2^31)";
    return nullptr;
}

}  // namespace dfh

// =================================================================================== C ABI
extern "C" {

size_t dfh_pool_features_workspace_bytes(long n_pixels, long n_verts) {
    if (dfh::pool_check_sizes(n_pixels, 1, n_verts) || n_pixels == 0 || n_verts == 0) return 0;
    return dfh::pool_layout(n_pixels, n_verts).end;
}

int dfh_pool_features_tile(int tile[4]) {
    using namespace dfh;
    DFH_REQUIRE(tile, "dfh_pool_features_tile: null output");
    tile[0] = kPoolBlock;
    tile[1] = kPoolScanChunk;
    tile[2] = kPoolCap;
    tile[3] = kPoolBigStep;
    return DFH_OK;
}

int dfh_pool_features(const int *vid, const float *feat, long n_pixels, int dim, long n_verts, float *feat_out, int *cnt_out,
                      void *workspace, size_t workspace_bytes, void *stream) {
    using namespace dfh;
    const char *bad = pool_check_sizes(n_pixels, dim, n_verts);
    DFH_REQUIRE(!bad, "dfh_pool_features: %s (n_pixels=%ld, dim=%d, n_verts=%ld)", bad, n_pixels, dim, n_verts);
    DFH_REQUIRE(n_pixels == 0 || (vid && feat), "dfh_pool_features: null input");
    DFH_REQUIRE(n_verts == 0 || (feat_out && cnt_out), "dfh_pool_features: null output");
    const bool work = n_pixels > 0 && n_verts > 0;
    PoolLayout L;
    if (work) {
        L = pool_layout(n_pixels, n_verts);
        DFH_REQUIRE(workspace, "dfh_pool_features: null workspace");
        DFH_REQUIRE(workspace_bytes >= L.end, "dfh_pool_features: workspace too small (%zu < %zu bytes)", workspace_bytes, L.end);
        DFH_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "dfh_pool_features: workspace must be 16-byte aligned");
    }
    if (n_verts == 0) return DFH_OK;
    hipStream_t s = (hipStream_t)stream;
    DFH_HIP_CHECK(hipMemsetAsync(cnt_out, 0, 4 * (size_t)n_verts, s));
    if (!work) {
        DFH_HIP_CHECK(hipMemsetAsync(feat_out, 0, 4 * (size_t)n_verts * dim, s));
        return DFH_OK;
    }
    char *ws = static_cast<char *>(workspace);
    int *local = reinterpret_cast<int *>(ws + L.local);
    int *chunk_tot = reinterpret_cast<int *>(ws + L.chunk_tot);
    int *chunk_base = reinterpret_cast<int *>(ws + L.chunk_base);
    int *big_n = reinterpret_cast<int *>(ws + L.big_n);
    int *big = reinterpret_cast<int *>(ws + L.big);
    int *slot = reinterpret_cast<int *>(ws + L.slot);
    int *list = reinterpret_cast<int *>(ws + L.list);
    const PoolSegs segs = {local, chunk_base};
    DFH_HIP_CHECK(hipMemsetAsync(big_n, 0, sizeof(int), s));
    const dim3 block(kPoolBlock);
    const dim3 pix_grid((unsigned)((n_pixels + kPoolBlock - 1) / kPoolBlock));
    hipLaunchKernelGGL(pool_count_kernel, pix_grid, block, 0, s, vid, n_pixels, n_verts, cnt_out, slot);
    hipLaunchKernelGGL((scan_chunks_kernel<int, int, kPoolWaves>), dim3((unsigned)L.nchunks), block, 0, s, (const int *)cnt_out, n_verts, local,
                       chunk_tot);
    hipLaunchKernelGGL((scan_chunk_totals_kernel<int, kPoolWaves>), dim3(1), block, 0, s, (const int *)chunk_tot, L.nchunks, chunk_base,
                       (int *)nullptr);
    hipLaunchKernelGGL(pool_scatter_kernel, pix_grid, block, 0, s, vid, n_pixels, n_verts, segs, (const int *)slot, list);
    hipLaunchKernelGGL(pool_order_kernel, dim3((unsigned)((n_verts + kPoolWaves - 1) / kPoolWaves)), block, 0, s, n_verts,
                       (const int *)cnt_out, segs, list, big_n, big);
    const long big_grid = L.big_cap < 1024 ? L.big_cap : 1024;                      // the long segments' count stays on the device
    hipLaunchKernelGGL(pool_order_big_kernel, dim3((unsigned)big_grid), block, 0, s, vid, (const int *)cnt_out, segs, list,
                       (const int *)big_n, (const int *)big);
    const int per = kPoolBlock / dim;
    hipLaunchKernelGGL(pool_sum_kernel, dim3((unsigned)((n_verts + per - 1) / per)), block, 0, s, feat, dim, n_verts, (const int *)cnt_out,
                       segs, (const int *)list, feat_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

}  // extern "C"
