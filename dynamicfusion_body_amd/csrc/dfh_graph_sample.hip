// Greedy radius subsampling (reference core/util.py:27-47) on the device: dfh_radius_sample.
//
// The reference takes the first remaining candidate, drops every candidate closer than `radius` to it and repeats.  Its
// result is the lexicographically first maximal independent set of the graph "closer than radius":
//      i is selected  <=>  no selected j < i has dist(p_i, p_j) < radius,
// and that set is built here in parallel rounds, index for index the host loop's output.
//
// One round, over a uniform cell table whose cell side is at least `radius` (so the 3 x 3 x 3 cells around a point hold every
// point closer than `radius` to it -- "Coverage" below):
//   select   an undecided point is selected iff it is the lowest undecided index of its 27 cells.  Every lower index that
//            could still reject it lies in those cells and is decided, and the decided ones that were selected have already
//            rejected what they reach: nothing selected lies within the radius, so the greedy rule selects it too.
//   reject   an undecided point closer than `radius` (the reference's expression, strict) to a point selected in THIS round
//            is rejected.  A cell yields at most one selected point per round, its lowest undecided index, which is what
//            the cell's table entry holds: the 27 entries around a point are all it has to test.
//            The points still undecided enter their index into the next round's table (an atomic minimum per cell).
// Selection is only ever delayed by the cells being a superset of the ball, never wrong; the lowest undecided index of the
// whole input is selected in every round, so at most n_points rounds run.
//
// Tables: two, used alternately (reject of round r fills the table of round r + 1 while its own threads still read the
// table of round r).  An entry is (~round << 32 | index), so that an entry of an older round compares above every entry of
// the current one and reads as "empty": no table is cleared between rounds.  Rounds count from 1; 0xff..ff is "empty".
//
// Control flow: every round is two launches on the stream; no workgroup waits for another.  The host queues kBatch rounds (a
// round with nothing undecided is a no-op), then reads the rounds' undecided counts from pinned host memory.
//
// Coverage under rounding.  Let dist(p, q) < radius as computed (fp64, operation by operation).  On every axis the computed
// difference d satisfies |d| <= dist (1 + 2^-51): d * d is a term of a sum of non-negative terms and rounding is monotone,
// (unless d * d underflows, |d| < 2^-511, which the floor of 2^-500 on the cell side covers), and the real difference is
// within 2^-53 relative of d.  So the real per-axis gap is below radius (1 + 2^-50), while side >= radius (1 + 2^-20).
// A cell coordinate is floor(fl(fl(p - lo) / side)): two roundings, relative error 2^-52 of a value below the table's extent
// (at most 2^21 cells on an axis), i.e. at most 2^-31 absolute.  Two points whose real gap is below side (1 - 2^-21) get
// computed coordinates that differ by less than 1 - 2^-21 + 2^-30 < 1 before the floor, so their cells are equal or adjacent;
// the clamp to the table is monotone and keeps that.  Enlarging the side (to fit the table, "one far outlier") keeps it too.
#include <cmath>

#include "dfh_common.h"
#include "dfh_scan.h"

namespace dfh {

constexpr int kRsBatch = 8;                    // rounds queued between two reads of the undecided counts
constexpr long kRsMaxCells = 1L << 21;         // table cap: cells grow beyond `radius` to fit the bounding box into it
constexpr int kRsBoxBlocks = 1024;
constexpr unsigned long long kRsEmpty = ~0ull;

struct RsGrid {                                // written by rs_grid_kernel, read by every later launch
    double lo[3];
    double side;
    int dim[3];
    int pad;
};

enum : unsigned char { kRsUndecided = 0, kRsSelected = 1, kRsRejected = 2 };

__host__ __device__ inline long rs_cells(long n) {          // table size: a function of n_points only
    long c = 4096;
    while (c < 2 * n && c < kRsMaxCells) c *= 2;
    return c;
}

// ---- workspace layout (all offsets multiples of 8 bytes) -----------------------------------------------------------------
struct RsLayout {
    size_t grid, und, total, box, table0, table1, cell, state, blk, end;
};

static RsLayout rs_layout(long n) {
    RsLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 7) / 8 * 8; return at; };
    const size_t cells = (size_t)rs_cells(n);
    L.grid = take(sizeof(RsGrid));
    L.und = take(sizeof(unsigned long long) * kRsBatch);
    L.total = take(sizeof(long));
    L.box = take(sizeof(double) * 6 * kRsBoxBlocks);
    L.table0 = take(sizeof(unsigned long long) * cells);
    L.table1 = take(sizeof(unsigned long long) * cells);
    L.cell = take(sizeof(int) * (size_t)n);
    L.state = take((size_t)n);
    L.blk = take(sizeof(long) * (((size_t)n + 255) / 256));
    L.end = o;
    return L;
}

// ---- bounding box: per-workgroup minima of (x, y, z, -x, -y, -z), then one workgroup finishes and lays out the grid --------
__device__ __forceinline__ void rs_block_min6(double (&v)[6], double (*sred)[4], double *out) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[c] = fmin(v[c], __shfl_xor(v[c], o, 64));
        if (lane == 0) sred[c][wv] = v[c];
    }
    __syncthreads();
    if (threadIdx.x < 6) out[threadIdx.x] = fmin(fmin(sred[threadIdx.x][0], sred[threadIdx.x][1]), fmin(sred[threadIdx.x][2], sred[threadIdx.x][3]));
}

__global__ __launch_bounds__(256) void rs_box_kernel(const double *__restrict__ pts, long n, double *__restrict__ partial) {
    __shared__ double sred[6][4];
    const double big = __builtin_huge_val();
    double v[6] = {big, big, big, big, big, big};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        v[0] = fmin(v[0], x); v[1] = fmin(v[1], y); v[2] = fmin(v[2], z);
        v[3] = fmin(v[3], -x); v[4] = fmin(v[4], -y); v[5] = fmin(v[5], -z);
    }
    rs_block_min6(v, sred, partial + 6 * (size_t)blockIdx.x);
}

__global__ __launch_bounds__(256) void rs_grid_kernel(const double *__restrict__ partial, int rows, double radius, long cells,
                                                       RsGrid *__restrict__ grid) {
    __shared__ double sred[6][4];
    __shared__ double box[6];
    const double big = __builtin_huge_val();
    double v[6] = {big, big, big, big, big, big};
    for (int r = threadIdx.x; r < rows; r += 256)
#pragma unroll
        for (int c = 0; c < 6; ++c) v[c] = fmin(v[c], partial[6 * (size_t)r + c]);
    rs_block_min6(v, sred, box);
    __syncthreads();
    if (threadIdx.x != 0) return;
    // side: above the radius by 2^-20 relative (see "Coverage" at the top), never below 2^-500; doubled until the box fits the table.
    // A box that never fits (an extent that is not finite): one cell, which is a superset of everything.
    double side = fmax(radius * (1.0 + 0x1p-20), 0x1p-500);
    const double ext[3] = {-box[3] - box[0], -box[4] - box[1], -box[5] - box[2]};
    double d[3] = {1.0, 1.0, 1.0};
    bool fits = false;
    for (int it = 0; it < 2200 && !fits; ++it) {
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = fmax(floor(ext[a] / side) + 1.0, 1.0);       // (fmax drops a NaN: at least one cell)
        fits = d[0] * d[1] * d[2] <= (double)cells;
        if (!fits) side *= 2.0;
    }
    if (!fits) d[0] = d[1] = d[2] = 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { grid->lo[a] = box[a]; grid->dim[a] = (int)d[a]; }
    grid->side = side;
    grid->pad = 0;
}

// cell coordinate on one axis; fmax / fmin drop a NaN, so whatever the coordinate is the result lies inside the table
__device__ __forceinline__ int rs_coord(double p, double lo, double side, int dim) {
    const double u = floor((p - lo) / side);
    return (int)fmin(fmax(u, 0.0), (double)(dim - 1));
}

__device__ __forceinline__ unsigned long long rs_key(unsigned round, long i) {
    return ((unsigned long long)(~round) << 32) | (unsigned long long)(unsigned)i;
}

// every point: its cell, state "undecided", and its index into the table of round 1
__global__ __launch_bounds__(256) void rs_bin_kernel(const double *__restrict__ pts, long n, const RsGrid *__restrict__ grid,
                                                      int *__restrict__ cell, unsigned char *__restrict__ state,
                                                      unsigned long long *__restrict__ table) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const RsGrid g = *grid;
    const int cx = rs_coord(pts[3 * (size_t)i], g.lo[0], g.side, g.dim[0]);
    const int cy = rs_coord(pts[3 * (size_t)i + 1], g.lo[1], g.side, g.dim[1]);
    const int cz = rs_coord(pts[3 * (size_t)i + 2], g.lo[2], g.side, g.dim[2]);
    const int c = (cx * g.dim[1] + cy) * g.dim[2] + cz;
    cell[i] = c;
    state[i] = kRsUndecided;
    atomicMin(table + c, rs_key(1u, i));
}

// selected iff the lowest undecided index of the 27 cells around the point (table: this round's)
__global__ __launch_bounds__(256) void rs_select_kernel(long n, unsigned round, const RsGrid *__restrict__ grid,
                                                         const int *__restrict__ cell, unsigned char *__restrict__ state,
                                                         const unsigned long long *__restrict__ table) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || state[i] != kRsUndecided) return;
    const int c = cell[i];
    const unsigned long long mine = rs_key(round, i);
    if (table[c] != mine) return;                          // not even the lowest of its own cell
    const int ny = grid->dim[1], nz = grid->dim[2], nx = grid->dim[0];
    const int cz = c % nz, cy = (c / nz) % ny, cx = c / (nz * ny);
    bool lowest = true;
    for (int x = max(cx - 1, 0); x <= min(cx + 1, nx - 1); ++x)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, ny - 1); ++y)
            for (int z = max(cz - 1, 0); z <= min(cz + 1, nz - 1); ++z)
                lowest = lowest && table[(x * ny + y) * nz + z] >= mine;       // (older rounds' entries compare above)
    if (lowest) state[i] = kRsSelected;
}

// rejected iff closer than radius to a point selected in this round; otherwise still undecided: counted, and entered into
// the next round's table
__global__ __launch_bounds__(256) void rs_reject_kernel(const double *__restrict__ pts, long n, double radius, unsigned round,
                                                         const RsGrid *__restrict__ grid, const int *__restrict__ cell,
                                                         unsigned char *__restrict__ state,
                                                         const unsigned long long *__restrict__ table,
                                                         unsigned long long *__restrict__ table_next,
                                                         unsigned long long *__restrict__ undecided) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    bool open = i < n && state[i] == kRsUndecided;
    if (open) {
        const int c = cell[i];
        const int ny = grid->dim[1], nz = grid->dim[2], nx = grid->dim[0];
        const int cz = c % nz, cy = (c / nz) % ny, cx = c / (nz * ny);
        const double px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
        bool hit = false;
        for (int x = max(cx - 1, 0); x <= min(cx + 1, nx - 1) && !hit; ++x)
            for (int y = max(cy - 1, 0); y <= min(cy + 1, ny - 1) && !hit; ++y)
                for (int z = max(cz - 1, 0); z <= min(cz + 1, nz - 1) && !hit; ++z) {
                    const unsigned long long e = table[(x * ny + y) * nz + z];
                    if ((unsigned)(e >> 32) != ~round) continue;               // nothing undecided entered this cell this round
                    const size_t j = (size_t)(unsigned)e;
                    if (state[j] != kRsSelected) continue;                     // (states only leave "undecided" in this launch)
                    const double d0 = px - pts[3 * j], d1 = py - pts[3 * j + 1], d2 = pz - pts[3 * j + 2];
                    hit = sqrt((d0 * d0 + d1 * d1) + d2 * d2) < radius;        // core/util.py:43-44, operation by operation
                }
        if (hit) {
            state[i] = kRsRejected;
            open = false;
        } else {
            atomicMin(table_next + c, rs_key(round + 1u, i));
        }
    }
    const unsigned long long bal = __ballot(open);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(undecided, (unsigned long long)__popcll(bal));
}

// the batch's undecided counts into pinned host memory (plain stores; the host reads them after the stream has drained)
__global__ void rs_publish_kernel(const unsigned long long *__restrict__ und, unsigned long long *__restrict__ host, int n) {
    if ((int)threadIdx.x < n) host[threadIdx.x] = und[threadIdx.x];
}

// ---- output: the selected indices in ascending order (count per 256 points, scan, emit) ----------------------------------
__global__ __launch_bounds__(256) void rs_count_kernel(const unsigned char *__restrict__ state, long n, long *__restrict__ blk) {
    __shared__ int cnt[4];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long bal = __ballot(i < n && state[i] == kRsSelected);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// exclusive scan of blk[0..m) in place by one workgroup (dfh_scan.h's block_scan_rounds), the sum to total and to the host word
__global__ __launch_bounds__(1024) void rs_scan_kernel(long *__restrict__ blk, long m, long *__restrict__ total, long *__restrict__ total_host) {
    __shared__ long wtot[16];
    const long sum = block_scan_rounds<16, 1, long>(
        m, wtot, [&](long i) { return blk[i]; }, [&](long i, long at) { blk[i] = at; });
    if (threadIdx.x == 0) {
        *total = sum;
        *total_host = sum;
    }
}

__global__ __launch_bounds__(256) void rs_emit_kernel(const unsigned char *__restrict__ state, long n, const long *__restrict__ blk,
                                                       int *__restrict__ idx_out, long capacity) {
    __shared__ int cnt[4];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool sel = i < n && state[i] == kRsSelected;
    const unsigned long long bal = __ballot(sel);
    if (lane == 0) cnt[wv] = __popcll(bal);
    __syncthreads();
    long pos = blk[blockIdx.x] + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) pos += cnt[w];
    if (sel && pos < capacity) idx_out[pos] = (int)i;
}

// pinned host words the rounds' counts arrive in: one block per calling thread, kept for the life of the process
static unsigned long long *rs_host_words() {
    thread_local unsigned long long *h = nullptr;
    if (!h) {
        void *p = nullptr;
        if (hipHostMalloc(&p, sizeof(unsigned long long) * (kRsBatch + 1), hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        h = static_cast<unsigned long long *>(p);
    }
    return h;
}

}  // namespace dfh

// =================================================================================== C ABI
extern "C" {

size_t dfh_radius_sample_workspace_bytes(long n_points) {
    if (n_points <= 0 || n_points >= (1L << 31)) return 0;
    return dfh::rs_layout(n_points).end;
}

int dfh_radius_sample(const double *points, long n_points, double radius, int *idx_out, long capacity, long *count_out,
                      int *rounds_out, void *workspace, size_t workspace_bytes, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(n_points >= 0 && n_points < (1L << 31), "dfh_radius_sample: n_points=%ld outside [0, 2^31)", n_points);
    DFH_REQUIRE(std::isfinite(radius) && radius > 0.0, "dfh_radius_sample: radius must be finite and > 0");
    DFH_REQUIRE(capacity >= 0, "dfh_radius_sample: negative capacity");
    DFH_REQUIRE(count_out, "dfh_radius_sample: null count_out");
    if (n_points == 0) {
        *count_out = 0;
        if (rounds_out) *rounds_out = 0;
        return DFH_OK;
    }
    DFH_REQUIRE(points && idx_out && workspace, "dfh_radius_sample: null pointer");
    const long n = n_points;
    const RsLayout L = rs_layout(n);
    DFH_REQUIRE(workspace_bytes >= L.end, "dfh_radius_sample: workspace too small (%zu < %zu bytes)", workspace_bytes, L.end);
    DFH_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "dfh_radius_sample: workspace must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    RsGrid *grid = reinterpret_cast<RsGrid *>(ws + L.grid);
    unsigned long long *und = reinterpret_cast<unsigned long long *>(ws + L.und);
    long *total = reinterpret_cast<long *>(ws + L.total);
    double *box = reinterpret_cast<double *>(ws + L.box);
    unsigned long long *table[2] = {reinterpret_cast<unsigned long long *>(ws + L.table0), reinterpret_cast<unsigned long long *>(ws + L.table1)};
    int *cell = reinterpret_cast<int *>(ws + L.cell);
    unsigned char *state = reinterpret_cast<unsigned char *>(ws + L.state);
    long *blk = reinterpret_cast<long *>(ws + L.blk);
    unsigned long long *host = rs_host_words();
    if (!host) return fail(DFH_E_HIP, "dfh_radius_sample: no pinned host memory for the round counters");
    unsigned long long *host_dev = nullptr;
    DFH_HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void **>(&host_dev), host, 0));

    const long cells = rs_cells(n);
    const unsigned nblk = (unsigned)((n + 255) / 256);
    const int box_blocks = (int)(nblk < (unsigned)kRsBoxBlocks ? nblk : (unsigned)kRsBoxBlocks);
    // both tables "empty" (they are adjacent in the workspace)
    DFH_HIP_CHECK(hipMemsetAsync(table[0], 0xff, (L.table1 - L.table0) + sizeof(unsigned long long) * (size_t)cells, s));
    hipLaunchKernelGGL(rs_box_kernel, dim3(box_blocks), dim3(256), 0, s, points, n, box);
    hipLaunchKernelGGL(rs_grid_kernel, dim3(1), dim3(256), 0, s, box, box_blocks, radius, cells, grid);
    hipLaunchKernelGGL(rs_bin_kernel, dim3(nblk), dim3(256), 0, s, points, n, grid, cell, state, table[1]);      // round 1 reads table[1 & 1]
    DFH_HIP_CHECK(hipGetLastError());

    unsigned round = 1;
    int rounds = 0;
    unsigned long long open = (unsigned long long)n;
    while (open > 0) {
        DFH_HIP_CHECK(hipMemsetAsync(und, 0, sizeof(unsigned long long) * kRsBatch, s));
        for (int b = 0; b < kRsBatch; ++b, ++round) {
            unsigned long long *cur = table[round & 1u], *next = table[(round + 1u) & 1u];
            hipLaunchKernelGGL(rs_select_kernel, dim3(nblk), dim3(256), 0, s, n, round, grid, cell, state, cur);
            hipLaunchKernelGGL(rs_reject_kernel, dim3(nblk), dim3(256), 0, s, points, n, radius, round, grid, cell, state, cur, next, und + b);
        }
        hipLaunchKernelGGL(rs_publish_kernel, dim3(1), dim3(64), 0, s, und, host_dev, kRsBatch);
        DFH_HIP_CHECK(hipGetLastError());
        DFH_HIP_CHECK(hipStreamSynchronize(s));
        for (int b = 0; b < kRsBatch && open > 0; ++b) {
            const unsigned long long now = host[b];
            if (now >= open)                 // every round selects the lowest undecided index: this cannot happen
                return fail(DFH_E_INTERNAL, "dfh_radius_sample: round %d decided nothing (%llu points undecided)", rounds + 1, now);
            open = now;
            ++rounds;
        }
    }
    hipLaunchKernelGGL(rs_count_kernel, dim3(nblk), dim3(256), 0, s, state, n, blk);
    hipLaunchKernelGGL(rs_scan_kernel, dim3(1), dim3(1024), 0, s, blk, (long)nblk, total, reinterpret_cast<long *>(host_dev + kRsBatch));
    hipLaunchKernelGGL(rs_emit_kernel, dim3(nblk), dim3(256), 0, s, state, n, blk, idx_out, capacity);
    DFH_HIP_CHECK(hipGetLastError());
    DFH_HIP_CHECK(hipStreamSynchronize(s));
    *count_out = (long)host[kRsBatch];
    if (rounds_out) *rounds_out = rounds;
    return DFH_OK;
}

}  // extern "C"
