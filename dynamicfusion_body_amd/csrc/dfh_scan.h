// The exclusive prefix sum of a count -> scan -> emit pipeline, stated once for every file that has one (dfh_extract, dfh_pool,
// dfh_render's samples, dfh_mesh, dfh_plan, dfh_mesh_sdf, dfh_graph_sample).  Integer sums do not depend on the order of the
// additions, so every instance gives the bits a serial loop gives.  Which piece to use when:
//   wave_scan_inclusive / wave_scan_exclusive   one value per lane, inside one wave, no LDS and no barrier (a wave that owns a row)
//   block_scan_exclusive<WAVES>                 one value per thread of a 64 * WAVES workgroup: the prefix and the workgroup's sum in
//                                               every thread.  A kernel with a load/store shape of its own (16-byte packs, several
//                                               fields, an ordered compaction) does its loads, calls this, does its stores
//   block_scan_rounds<WAVES, ITEMS>             ONE workgroup scans a whole array in rounds through load / store callables and
//                                               returns the sum: the lists of a frame, a cell table, the totals of a two-level scan
//   scan_chunks_kernel + scan_chunk_totals_kernel   the two-level form for arrays too long for one workgroup: chunks scanned from
//                                               zero that leave their totals, then one workgroup over the totals; element e's prefix
//                                               is chunk_base[e / chunk] + local[e]
// A new count/scan/emit feature includes this header; it does not copy a kernel.
// Out of here on purpose: reductions (__shfl_down / __shfl_xor sums and minima) and the ballot-rank of one flag per lane.
#pragma once
#include "dfh_common.h"

namespace dfh {

// ------------------------------------------------------------------------------- one wave
// inclusive prefix over the 64 lanes: six shuffles (T = int, unsigned, long, unsigned long long)
template <typename T>
__device__ __forceinline__ T wave_scan_inclusive(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const T y = __shfl_up(v, o, kWave);
        if (lane >= o) v += y;
    }
    return v;
}

// exclusive prefix; total = the wave's sum, in every lane
template <typename T>
__device__ __forceinline__ T wave_scan_exclusive(T v, T &total) {
    const T inc = wave_scan_inclusive(v);
    total = __shfl(inc, kWave - 1, kWave);
    return inc - v;
}

// ------------------------------------------------------------------------------- one workgroup of 64 * WAVES threads
// Exclusive prefix of one value per thread; total = the workgroup's sum, in every thread (a carry across rounds is a register).
// wtot: WAVES entries of LDS.  One barrier.  A caller that calls again with the same wtot puts a __syncthreads() between the
// calls (the next call rewrites what slower waves may still read); a caller that does not reuse it takes none.
// UNROLL: the walk over the wave totals, unrolled in full by default (WAVES reads in flight at once).  UNROLL = 1 passes them
// through one register, for a caller that holds many values of its own across the call: with its sixteen counts a thread and
// sixteen totals in flight plan_scan2_kernel took 75 VGPRs and lost two waves per SIMD, rolled it takes 53 (54 before).
template <int WAVES, int UNROLL = WAVES, typename T>
__device__ __forceinline__ T block_scan_exclusive(T v, T *wtot, T &total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const T inc = wave_scan_inclusive(v);
    if (lane == kWave - 1) wtot[wv] = inc;
    __syncthreads();
    T off = 0, all = 0;
#pragma unroll UNROLL
    for (int w = 0; w < WAVES; ++w) {
        const T n = wtot[w];
        off += w < wv ? n : 0;
        all += n;
    }
    total = all;
    return off + inc - v;
}

// One workgroup scans n values in rounds of 64 * WAVES * ITEMS: store(i, prefix of element i) for every i < n, from
// v = load(i); returns the sum in every thread.  A thread holds up to ITEMS consecutive values in registers; a round that is
// not full spreads what is left evenly, so a short array still uses every wave.  load and store may touch the same array (each
// element is loaded by the thread that stores it, before it does) and store may write several arrays or narrow the value.
// Two barriers a round, the carry in a register.
template <int WAVES, int ITEMS, typename T, typename Index, typename Load, typename Store>
__device__ __forceinline__ T block_scan_rounds(Index n, T *wtot, Load load, Store store) {
    constexpr Index kRound = (Index)(kWave * WAVES) * ITEMS;
    T carry = 0;
    for (Index base = 0; base < n; base += kRound) {
        const Index left = n - base < kRound ? n - base : kRound;
        const int per = ITEMS == 1 ? 1 : (int)((left + kWave * WAVES - 1) / (kWave * WAVES));      // values per thread, this round
        const Index i0 = base + (Index)threadIdx.x * per;
        T v[ITEMS];
        T sum = 0;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            v[j] = (j < per && i0 + j < n) ? (T)load(i0 + j) : (T)0;
            sum += v[j];
        }
        T all;
        T run = carry + block_scan_exclusive<WAVES, (ITEMS > 1 ? 1 : WAVES)>(sum, wtot, all);
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            if (j < per && i0 + j < n) store(i0 + j, run);
            run += v[j];
        }
        carry += all;
        __syncthreads();                                     // wtot is rewritten by the next round
    }
    return carry;
}

// ------------------------------------------------------------------------------- the two-level pair
// Workgroup c scans counts [c * chunk, (c + 1) * chunk) from zero, chunk = 256 * WAVES (a thread takes four consecutive counts):
// local[e] = the counts of e's chunk in front of e, chunk_tot[c] = the chunk's sum (< 2^31 inside a chunk: CountT; TotalT holds
// the sum of all).
template <typename CountT, typename TotalT, int WAVES>
__global__ __launch_bounds__(kWave * WAVES) void scan_chunks_kernel(const CountT *__restrict__ cnt, long n, CountT *__restrict__ local,
                                                                    TotalT *__restrict__ chunk_tot) {
    __shared__ CountT wtot[WAVES];
    const long base = (long)blockIdx.x * (4 * kWave * WAVES) + 4 * (long)threadIdx.x;
    CountT v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = base + j < n ? cnt[base + j] : 0;
    CountT all;
    const CountT ex = block_scan_exclusive<WAVES>((CountT)((v[0] + v[1]) + (v[2] + v[3])), wtot, all);
    const CountT o4[4] = {ex, ex + v[0], ex + v[0] + v[1], ex + v[0] + v[1] + v[2]};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (base + j < n) local[base + j] = o4[j];
    if (threadIdx.x == 0) chunk_tot[blockIdx.x] = (TotalT)all;
}

// ONE workgroup: chunk_base[c] = the totals in front of chunk c; with total_out also chunk_base[nchunks] = *total_out = the sum
template <typename TotalT, int WAVES>
__global__ __launch_bounds__(kWave * WAVES) void scan_chunk_totals_kernel(const TotalT *__restrict__ chunk_tot, long nchunks,
                                                                          TotalT *__restrict__ chunk_base, TotalT *__restrict__ total_out) {
    __shared__ TotalT wtot[WAVES];
    const TotalT sum = block_scan_rounds<WAVES, 1, TotalT>(
        nchunks, wtot, [&](long i) { return chunk_tot[i]; }, [&](long i, TotalT at) { chunk_base[i] = at; });
    if (threadIdx.x == 0 && total_out) {
        chunk_base[nchunks] = sum;
        *total_out = sum;
    }
}

}  // namespace dfh
