// Block-Jacobi PCG on the 6x6 block-sparse normal equations, and the update dq <- exp(xi) (x) dq of every node.
//
// Two paths with the same iterates in exact arithmetic: one persistent launch for the whole solve (pcg_cg1_kernel, a
// single-reduction recurrence; taken when every row can have a co-resident wave of its own, pcg_shape) and two launches
// per iteration otherwise.  Neither has a floating-point atomic: every sum is added in a fixed order, the same bits every
// run and on every rank.  Restated in oracle/gn_np.py.
#include "dfh_pcg.h"

#include "dfh_solve_math.h"

namespace dfh {

// ------------------------------------------------------------------------------- PCG
// Solves (A + lm_abs I + lm_rel diag(A)) x = -rhs with block-Jacobi preconditioning.
struct PcgParams {
    int N;
    double lm_abs, lm_rel;
};

// The multi-launch path's dot products without atomics: every workgroup of the producing launch stores ONE partial (its waves'
// values added in a fixed order), every workgroup of the consuming launch adds all partials in the same fixed order -- the same
// bits in every workgroup, every run and on every rank (with atomicAdd the order, hence the last bits, changed from run to run).
__device__ __forceinline__ void wg_store_partial(double wave_value, double *slot) {     // all 256 threads; wave_value on lane 0
    __shared__ double s_part[4];
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = wave_value;
    __syncthreads();
    if (threadIdx.x == 0) slot[blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}
__device__ __forceinline__ double wg_sum_partials(const double *__restrict__ part, int n) {   // all 256 threads
    __shared__ double s_sum[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += part[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    const double v = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
    __syncthreads();
    return v;
}

__global__ __launch_bounds__(256) void pcg_init_kernel(const int *__restrict__ row_ptr, const int *__restrict__ col,
                                                        double *__restrict__ vals, const double *__restrict__ rhs,
                                                        const PcgParams p, double *__restrict__ Minv, double *__restrict__ x,
                                                        double *__restrict__ r, double *__restrict__ pv, double *__restrict__ rz_part) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    double rz = 0.0;
    if (a < p.N) {
    const int blk = find_block(row_ptr, col, a, a);
    double D[36];
    for (int i = 0; i < 36; ++i) D[i] = blk >= 0 ? vals[36 * (size_t)blk + i] : 0.0;
    for (int i = 0; i < 6; ++i) D[7 * i] = D[7 * i] + p.lm_abs + p.lm_rel * D[7 * i];
    if (blk >= 0) for (int i = 0; i < 6; ++i) vals[36 * (size_t)blk + 7 * i] = D[7 * i];     // damping lives in the matrix
    double Di[36];
    inv6(D, Di);
    for (int i = 0; i < 36; ++i) Minv[36 * (size_t)a + i] = Di[i];
    double rl[6], zl[6];
    for (int i = 0; i < 6; ++i) { rl[i] = -rhs[6 * a + i]; x[6 * a + i] = 0.0; r[6 * a + i] = rl[i]; }
    for (int i = 0; i < 6; ++i) {
        double z = 0.0;
        for (int j = 0; j < 6; ++j) z += Di[6 * i + j] * rl[j];
        zl[i] = z;
        pv[6 * a + i] = z;                 // z0; the first SpMV takes p = z (beta = 0)
        rz += rl[i] * z;
    }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rz += __shfl_xor(rz, o, 64);
    wg_store_partial(rz, rz_part);
}

// One 64-lane wave per node row: lane = (block slot b in 0..9) x (output component i in 0..5);
// each lane multiplies row i of its block with the 6 entries of p at the block's column node, the
// ten slots are folded with shuffles, lanes 0..5 hold y and lane 0 adds p.Ap once.
// The direction update p = z + beta p is folded in: every row forms its neighbours' new p on the
// fly from (z, p_prev, beta) and publishes its own new p in p_cur (ping-pong), so CG needs two
// launches per iteration.  scal_prev = {rz, pAp, rz_next} of the previous iteration (NULL: beta = 0).
__global__ __launch_bounds__(256) void pcg_spmv_kernel(const int *__restrict__ row_ptr, const int *__restrict__ col,
                                                        const double *__restrict__ vals, int N, const double *__restrict__ z,
                                                        const double *__restrict__ p_prev, double *__restrict__ p_cur,
                                                        double *__restrict__ Ap, const double *__restrict__ scal_prev,
                                                        double *__restrict__ scal, const double *__restrict__ rz_part, int n_rz_part,
                                                        double *__restrict__ pap_part) {
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.x * 4 + (threadIdx.x >> 6);
    // r.z of this iteration = the partials of the launch that produced z (init or the previous update), added here
    const double rz_now = wg_sum_partials(rz_part, n_rz_part);
    const double rz = scal_prev[0];                                     // the previous iteration's r.z (0 in iteration 0: beta = 0)
    const double beta = rz != 0.0 ? rz_now / rz : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) scal[0] = rz_now;         // rz of this iteration for update_xr and the next SpMV
    const bool row = a < N;
    const int slot = lane / 6, i = lane - 6 * slot;            // lanes 60..63: slot 10 (idle)
    double acc = 0.0;
    const int beg = row ? row_ptr[a] : 0, end = row ? row_ptr[a + 1] : 0;
    if (slot < 10) {
        for (int b = beg + slot; b < end; b += 10) {
            const double *B = vals + 36 * (size_t)b + 6 * i;
            const double *zj = z + 6 * col[b];
            const double *pj = p_prev + 6 * col[b];
            const double q0 = zj[0] + beta * pj[0], q1 = zj[1] + beta * pj[1], q2 = zj[2] + beta * pj[2];
            const double q3 = zj[3] + beta * pj[3], q4 = zj[4] + beta * pj[4], q5 = zj[5] + beta * pj[5];
            acc += ((B[0] * q0 + B[1] * q1) + (B[2] * q2 + B[3] * q3)) + (B[4] * q4 + B[5] * q5);
        }
    }
    double y = acc;
#pragma unroll
    for (int k = 1; k < 10; ++k) {
        const double o = __shfl(acc, lane + 6 * k, 64);
        y += (lane + 6 * k < 60) ? o : 0.0;
    }
    double contrib = 0.0;
    if (row && lane < 6) {
        const double pn = z[6 * a + lane] + beta * p_prev[6 * a + lane];
        p_cur[6 * a + lane] = pn;
        Ap[6 * a + lane] = y;
        contrib = pn * y;
    }
    contrib += __shfl_down(contrib, 4, 64);
    contrib += __shfl_down(contrib, 2, 64);
    contrib += __shfl_down(contrib, 1, 64);
    wg_store_partial(contrib, pap_part);                                 // p.Ap of this workgroup's four rows
}

// x += alpha p, r -= alpha Ap, z = Minv r, rz_next += r.z : one thread per unknown (6 per node; the
// node's six new residual entries are exchanged with shuffles inside the 6-lane group).
__global__ __launch_bounds__(256) void pcg_update_xr_kernel(int N, const double *__restrict__ Minv, double *__restrict__ x,
                                                             double *__restrict__ r, const double *__restrict__ pv,
                                                             const double *__restrict__ Ap, double *__restrict__ z,
                                                             const double *__restrict__ scal, const double *__restrict__ pap_part,
                                                             int n_pap_part, double *__restrict__ rz_part) {
    // 60 of the 64 lanes of a wave are used: 10 nodes per wave, 40 per block
    const int lane = threadIdx.x & 63;
    const int grp = lane / 6, i = lane - 6 * grp;
    const int a = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 10 + grp;
    const bool act = grp < 10 && a < N;
    const double rz = scal[0], pAp = wg_sum_partials(pap_part, n_pap_part);
    const double alpha = pAp != 0.0 ? rz / pAp : 0.0;
    double rn = 0.0;
    if (act) {
        const int u = 6 * a + i;
        x[u] += alpha * pv[u];
        rn = r[u] - alpha * Ap[u];
        r[u] = rn;
    }
    double zz = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double rj = __shfl(rn, 6 * grp + j, 64);
        if (act) zz += Minv[36 * (size_t)a + 6 * i + j] * rj;
    }
    double contrib = 0.0;
    if (act) { z[6 * a + i] = zz; contrib = rn * zz; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) contrib += __shfl_down(contrib, o, 64);
    wg_store_partial(contrib, rz_part);                                  // r.z of this workgroup's 40 rows (the next iteration's)
}

// ---- persistent PCG: the whole iteration loop in one launch --------------------------------------
// Every wave owns ONE node row for the whole solve: its 6x6 blocks (up to kRowCache per lane slot), its rows of the
// block-Jacobi inverse and its six entries of the CG vectors stay in registers; per iteration only the neighbours'
// published vectors are read (agent-scope loads) and ONE grid-wide reduction replaces the kernel boundaries.  The
// grid is sized so that all workgroups are co-resident (<= one per CU on at most half the CUs); every wait is bounded
// and an abort flag makes every wave leave if one ever times out (x is then NaN, never a hang).  Reductions: every
// workgroup adds its waves' values in LDS (fixed order) and publishes the partial; wave 0 reads all workgroups'
// partials and adds them in a fixed order: same bits every run and on every rank, no floating-point atomics, no
// counters, no cache-wide fences.  Measured (512 rows, tools/kbench_pcg.py): 3.0 us per iteration, of which ~1.8 us
// is the hand-off (stores becoming visible across the XCDs + one agent-scope load round trip of ~0.9 us).
constexpr int kRowCache = 3;               // blocks per lane slot held in registers (rows <= 30 blocks)
constexpr unsigned kSpinLimit = 1u << 22;  // default bound of a barrier's spin (~seconds); DFH_PCG_SPIN_LIMIT overrides (tests)
#ifndef DFH_PCG_POLL_GAP
#define DFH_PCG_POLL_GAP 1
#endif
#ifndef DFH_PCG_POLL_DELAY
#define DFH_PCG_POLL_DELAY 16
#endif
constexpr int kPollDelay = DFH_PCG_POLL_DELAY;   // s_sleep units (64 clocks) between a publish and the first look: a look costs a
                                                 // full round trip, one issued at once finds nothing (0 / 8 / 16 / 24 / 32: 4.25 / 3.73 / 3.45 / 3.63 / 3.83 us per iteration)
constexpr int kPollGap = DFH_PCG_POLL_GAP;       // s_sleep units (64 clocks) between two polls
constexpr int kMaxPcgBlocks = 512;         // persistent path only for grids up to this many workgroups

__device__ __forceinline__ double ld_agent(const double *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(double *p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- single-reduction PCG (Chronopoulos & Gear) -----------------------------------------------------------
// A grid-wide hand-off costs ~1.5-3 us across the eight XCDs (MI355X_MICROARCH.md, hand-off price list) and the
// textbook recurrence needs two reductions per iteration (p.Ap, then r.z).  This variant has ONE: with u = M^-1 r, w = A u,
//   gamma = r.u, delta = w.u  (both in the same reduction),  beta = gamma / gamma_old,
//   alpha = gamma / (delta - beta gamma / alpha_old),  p = u + beta p,  s = w + beta s  (= A p),
//   x += alpha p,  r -= alpha s,  u = M^-1 r,  w = A u.
// The exchange of the new u between rows would be a second synchronisation; it is avoided by linearity:
// u_new = u - alpha t with t = M^-1 s = v + beta t_old, v = M^-1 w, so every row publishes (u, v, t_old) BEFORE
// the reduction and its neighbours form its u_new themselves once alpha and beta are known -- with the same
// expression the owner uses, hence the same bits.  Same iterates as the textbook PCG in exact arithmetic.
//
// Hand-offs carry their own arrival flag.  Every published double (a workgroup's partial sums, a row's u, v, t) goes
// into a slot whose bits are all zero until the one 8-byte agent-scope store that fills it (a zero value is stored as
// -0.0), so a reader needs no barrier and the writer no store drain: it loads the slot and retries while the bits are
// zero.  The neighbours' (u, v, t) are requested right after a wave's own stores, i.e. while the reduction is still in
// flight, so an iteration's critical path is one store becoming visible plus one load (it was: drain the stores,
// publish the partial, poll the partials, then load the neighbours -- four trips).
//   * partial sums: a fresh pair of slots per workgroup and reduction (zeroed by the launch's memset);
//   * vectors: a ring of four phase regions {u, v, t} x 6N (zeroed by the memset); iteration `it` reads region it % 4
//     and publishes into (it + 1) % 4.  A row's wave clears its own entries of region (it - 1) % 4 after reduction `it`:
//     every reader was finished with them before it contributed to that reduction.  The wave's wait for its neighbours'
//     values in iteration it + 1 (loads issued after the clearing stores; vmcnt counts in issue order) proves the
//     clears complete; only then does the wave contribute to reduction it + 2 and later store the region's next
//     values (phase it + 3).  A reader asks for those only after it has seen reduction it + 2 complete, so it finds
//     zero bits or the new value, never the value of four phases ago.
// A wave whose wait runs out (spin_limit) or that sees the abort flag poisons its row with NaN: the NaN reaches every
// row through the next reduction, so x is NaN everywhere and nothing hangs.
struct BarrierLds2 {
    double wave_part[2][16];
    double total[2];
};
struct alignas(16) WaveLds {             // one wave's scratch for trading values between its lanes
    double q[kRowCache][64];
    double part[6][10];
    double w[6];
};
// orders a wave's LDS writes before its following LDS reads (the hardware executes one wave's LDS operations in
// order; this only keeps the compiler from moving them)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

__device__ __forceinline__ double nz_bits(double v) { return __double_as_longlong(v) == 0 ? -0.0 : v; }
__device__ __forceinline__ bool arrived(double v) { return __double_as_longlong(v) != 0; }

// workgroup barrier for LDS traffic only: vector-memory operations stay in flight across it
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Wave-wide sums without the LDS crossbar: DPP row shifts (lanes without a source add 0), then the two cross-row
// broadcasts; the total is read from lane 63 into scalar registers, i.e. the result is wave-uniform.  Fixed order.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp0_f64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xf, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double readlane_f64(double v, int l) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
    v += dpp0_f64<0x111>(v);                 // row_shr:1
    v += dpp0_f64<0x112>(v);                 // row_shr:2
    v += dpp0_f64<0x114>(v);                 // row_shr:4
    v += dpp0_f64<0x118>(v);                 // row_shr:8   -> lane 15 of every row: the row's sum
    v += dpp0_f64<0x142, 0xa>(v);            // row_bcast:15 into rows 1 and 3
    v += dpp0_f64<0x143, 0xc>(v);            // row_bcast:31 into rows 2 and 3
    return readlane_f64(v, 63);
}
__device__ __forceinline__ double sum6_f64(double v) {         // lanes 0..5 -> wave-uniform
    v += dpp0_f64<0x111>(v);
    v += dpp0_f64<0x112>(v);
    v += dpp0_f64<0x114>(v);
    return readlane_f64(v, 5);
}

struct PcgAbort {
    unsigned *flag;                      // this solve's abort flag (zero before the launch); flag[1]: "already counted"
    unsigned long long *count;           // the library's sticky per-device counter of timed-out solves
    unsigned *host_flag;                 // word in pinned host memory, set when the counter is bumped (dfh_pcg_status_peek)
    unsigned spin_limit;
    __device__ __forceinline__ bool raised() const { return __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u; }
    __device__ __forceinline__ void raise() const {                                        // one count per timed-out solve
        __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (atomicExch(flag + 1, 1u) == 0u) {
            atomicAdd(count, 1ull);
            if (host_flag) __hip_atomic_store(host_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
};

#ifdef DFH_PCG_TRACE     // experiment builds only (tools/build_variant.sh): wall-clock stamps of one wave's iteration phases
__device__ unsigned long long g_pcg_trace[64][16][12];
#define PCG_STAMP(k) do { if (lane == 0 && tw >= 0 && it < 16) { g_pcg_trace[tw][it][k] = wall_clock64(); if (k == 0) { g_pcg_trace[tw][it][9] = clock64(); g_pcg_trace[tw][it][10] = ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) | (unsigned)__builtin_amdgcn_s_getreg(63492); } } } while (0)
#define GS_STAMP(k) do { if ((threadIdx.x & 63) == 0 && tr) tr[k] = wall_clock64(); } while (0)
#define PRO_STAMP(k) do { __builtin_amdgcn_s_waitcnt(0); if ((threadIdx.x & 63) == 0 && (threadIdx.x >> 6) == (DFH_PCG_TRACE) && blockIdx.x < 64) g_pcg_trace[blockIdx.x][15][k] = wall_clock64(); } while (0)
#else
#define PCG_STAMP(k) do {} while (0)
#define GS_STAMP(k) do {} while (0)
#define PRO_STAMP(k) do {} while (0)
#endif

// Two grid-wide sums in one pass; slots = 2 * gridDim.x doubles (workgroup b: 2b, 2b+1), zero bits before the launch.
// in_flight() runs in every wave between the publish and the wait: loads issued there travel beside the reduction.
// Returns NaN totals when the wait was given up.
template <class R, class H>
__device__ __forceinline__ void grid_sum2(double *slots, const PcgAbort &ab, BarrierLds2 *lds, double v0, double v1 /* wave-uniform */,
                                          double *s0, double *s1, bool fetch, R &&request, H &&here, int blk, int nblk,
                                          unsigned long long *tr = nullptr) {
    // fetch: the wave also wants its neighbours' published values: request() issues the loads, here() says whether the
    // last request found them all (wave-uniform).  Every wave keeps asking while the reduction is in flight, so the
    // values and the totals are usually both there one load latency after the slowest workgroup's stores land.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    if (lane == 0) { lds->wave_part[0][wave] = v0; lds->wave_part[1][wave] = v1; }
    lds_barrier();
    GS_STAMP(5);
#ifdef DFH_PCG_TRACE
    if (tr && lane == 0) tr[8] = 0ull;
#endif
    if (wave == 0 && lane < 2) {
        double v = 0.0;
        for (int w = 0; w < waves; ++w) v += lds->wave_part[lane][w];
        st_agent(slots + 2 * blk + lane, nz_bits(v));
    }
    bool have = !fetch;
    GS_STAMP(6);
    unsigned spins = 0;
    if (kPollDelay > 0) __builtin_amdgcn_s_sleep(kPollDelay);   // nothing can have arrived yet
    if (wave == 0) {
        const int nb = nblk;                            // lane l adds workgroups l, l + 64, ...
        double t0 = 0.0, t1 = 0.0;
        for (;;) {
            bool all = true;
            t0 = 0.0;
            t1 = 0.0;
            for (int b = lane; b < nb; b += 64) {
                const double p0 = ld_agent(slots + 2 * b), p1 = ld_agent(slots + 2 * b + 1);
                all = all && arrived(p0) && arrived(p1);
                t0 += p0;
                t1 += p1;
            }
            if (!have) {
                request();
                have = here();
            }
            if (__all(all)) break;
#ifdef DFH_PCG_TRACE
            if (tr && lane == 0) tr[8] += 1ull;                 // failed polls
#endif
            if (++spins > ab.spin_limit || ab.raised()) {
                if (lane == 0) ab.raise();
                t0 = t1 = __builtin_nan("");
                break;
            }
            __builtin_amdgcn_s_sleep(kPollGap);
        }
        t0 = wave_sum_f64(t0);
        t1 = wave_sum_f64(t1);
        GS_STAMP(7);
        if (lane == 0) { lds->total[0] = t0; lds->total[1] = t1; }
    } else {
        while (!have) {
            request();
            have = here();
            if (have) break;
            if (++spins > ab.spin_limit || ab.raised()) {      // (the caller's wait sees the flag and poisons the row)
                if (lane == 0) ab.raise();
                break;
            }
            __builtin_amdgcn_s_sleep(kPollGap);
        }
    }
    lds_barrier();
    *s0 = lds->total[0];
    *s1 = lds->total[1];
}

// MAXT = largest workgroup it is launched with: 512 leaves 256 VGPRs per lane (no spills in the prologue's 6x6 inverse)
template <int MAXT>
__global__ __launch_bounds__(MAXT) void pcg_cg1_kernel(const int *__restrict__ row_ptr, const int *__restrict__ col, double *vals,
                                                        const double *__restrict__ rhs, const PcgParams prm, int iters,
                                                        double *__restrict__ x, double *ring /* 4 x {u, v, t} x 6N */, double *part,
                                                        unsigned *abort_flag, unsigned spin_limit, unsigned long long *abort_count,
                                                        unsigned *abort_host, double *__restrict__ update_dq, double update_step,
                                                        int die_stride) {
    // die_stride > 1 (experiment, option pcg_one_xcd): the grid is die_stride times too large and only the workgroups whose index
    // is a multiple of it work -- with round-robin dispatch over the eight XCDs (stride 8) they all sit on ONE die; the others leave
    if (die_stride > 1 && (blockIdx.x % die_stride) != 0) return;
    const int blk = die_stride > 1 ? (int)blockIdx.x / die_stride : (int)blockIdx.x;
    const int nblk = die_stride > 1 ? (int)gridDim.x / die_stride : (int)gridDim.x;
    if (die_stride > 1 && threadIdx.x == 0)                                     // which dies really took part (bit = XCC_ID): flag[3]
        atomicOr(abort_flag + 3, 1u << (__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) & 15));
    // update_dq != NULL: the row's wave also applies its twist, update_dq[a] <- exp(update_step * x_a) (x) update_dq[a]
    // abort_count is read by dfh_pcg_status() at the caller's next synchronisation point
    __shared__ BarrierLds2 lds;
    __shared__ WaveLds wlds[MAXT / 64];
    const PcgAbort ab{abort_flag, abort_count, abort_host, spin_limit};
    const int N = prm.N;
    const size_t N6 = 6 * (size_t)N;
    const int lane = threadIdx.x & 63;
    const int waves = blockDim.x >> 6;
    const int a = blk * waves + (threadIdx.x >> 6);
    const bool row = a < N;
    const int slot = lane / 6, i = lane - 6 * slot;            // lanes 60..63 idle in the SpMV
    const int beg = row ? row_ptr[a] : 0, end = row ? row_ptr[a + 1] : 0;
    const bool lead = row && lane < 6;
    const double rhs_i = lead ? rhs[6 * a + lane] : 0.0;      // (asked for now: needed after the 6x6 inverse)
    PRO_STAMP(0);
    // register cache of this row's blocks: lane (slot, i) holds row i of blocks beg+slot+10c; the diagonal block gets
    // its damping here (the damping lives in the matrix: it is also written back below)
    double Bc[kRowCache][6];
    int cj[kRowCache];
#pragma unroll
    for (int c = 0; c < kRowCache; ++c) {
        const int b = beg + slot + 10 * c;
        const bool have = slot < 10 && b < end;
        cj[c] = have ? col[b] : -1;
#pragma unroll
        for (int j = 0; j < 6; ++j) Bc[c][j] = have ? vals[36 * (size_t)b + 6 * i + j] : 0.0;
        if (have && cj[c] == a) {
#pragma unroll
            for (int j = 0; j < 6; ++j)                         // (static indices: a lane-dependent one would move Bc to scratch memory)
                if (j == i) {
                    Bc[c][j] = Bc[c][j] + prm.lm_abs + prm.lm_rel * Bc[c][j];
                    vals[36 * (size_t)b + 7 * i] = Bc[c][j];   // (only this lane reads that element, and it has)
                }
        }
    }
    PRO_STAMP(1);
    // block-Jacobi preconditioner: the damped diagonal block, from the register cache when it is there (six lanes hold
    // its rows: 36 shuffles instead of a binary search and a reload), else found and loaded the slow way
    double D[36];
    bool cached = false;
#pragma unroll
    for (int c = 0; c < kRowCache; ++c) {
        const unsigned long long m = __ballot(row && slot < 10 && cj[c] == a);
        if (m != 0ull && !cached) {                            // (wave-uniform)
            const int base = __ffsll((long long)m) - 1;        // lane (slot_d, 0)
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int j = 0; j < 6; ++j) D[6 * r + j] = __shfl(Bc[c][j], base + r, 64);
            cached = true;
        }
    }
    if (!cached) {
        const int dblk = lead ? find_block(row_ptr, col, a, a) : -1;
        __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
        for (int t = 0; t < 36; ++t) D[t] = dblk >= 0 ? vals[36 * (size_t)dblk + t] : 0.0;
#pragma unroll
        for (int t = 0; t < 6; ++t) D[7 * t] = D[7 * t] + prm.lm_abs + prm.lm_rel * D[7 * t];
        __builtin_amdgcn_s_waitcnt(0);                          // every read of the undamped diagonal has returned
        if (dblk >= 0) {
            double dv = D[0];
#pragma unroll
            for (int rr = 1; rr < 6; ++rr) dv = lane == rr ? D[7 * rr] : dv;
            vals[36 * (size_t)dblk + 7 * lane] = dv;
        }
    }
    PRO_STAMP(2);
    double Mi[6];
    {
        double mr[6];
        inv6_row(D, lane < 6 ? lane : 0, mr);                   // every lane runs the factorisation: same cost as one lane
#pragma unroll
        for (int j = 0; j < 6; ++j) Mi[j] = lead ? mr[j] : 0.0;
    }
    PRO_STAMP(3);
    // The neighbours' published values of this lane's cached blocks (element i of node cj[c]); rows wider than the
    // cache read the rest of their neighbours one at a time (wait_for).
    double nu[kRowCache], nv[kRowCache], nt[kRowCache];
    const bool wide = __any(slot < 10 && beg + slot + 10 * kRowCache < end);
    auto request = [&](const double *P, bool with_vt) {
#pragma unroll
        for (int c = 0; c < kRowCache; ++c) {
            const bool have = cj[c] >= 0;
            const size_t j6 = 6 * (size_t)(have ? cj[c] : 0) + i;
            nu[c] = have ? ld_agent(P + j6) : 1.0;
            nv[c] = have && with_vt ? ld_agent(P + N6 + j6) : 1.0;
            nt[c] = have && with_vt ? ld_agent(P + 2 * N6 + j6) : 1.0;
        }
    };
    auto all_here = [&]() {
        bool all = true;
#pragma unroll
        for (int c = 0; c < kRowCache; ++c) all = all && arrived(nu[c]) && arrived(nv[c]) && arrived(nt[c]);
        return __all(all) != 0;
    };
    bool mine = true;                                           // false once one of this wave's waits was given up
    auto await = [&](const double *P, bool with_vt) {          // checks the last request first
        unsigned spins = 0;
        while (!all_here()) {
            if (++spins > spin_limit || ab.raised()) {
                if (lane == 0) ab.raise();
                mine = false;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
            request(P, with_vt);
        }
    };
    auto wait_for = [&](const double *p) {                      // one published value (wide rows' tail)
        double v = ld_agent(p);
        unsigned spins = 0;
        while (!arrived(v)) {
            if (++spins > spin_limit || ab.raised()) {
                ab.raise();
                mine = false;
                return __builtin_nan("");
            }
            __builtin_amdgcn_s_sleep(1);
            v = ld_agent(p);
        }
        return v;
    };
    // y = A q for this row: qc[c] = element i of neighbour cj[c]'s vector, tail(j6) = element j6 of the vector for the
    // blocks beyond the cache.  Lanes trade values through the wave's own LDS scratch (a write, then wide reads: a
    // quarter of the instructions the cross-lane shuffles took): the six lanes of a slot read that neighbour's six
    // elements, lane i < 6 then reads and adds the ten slots' row-i partial sums (in slot order).  Result in lanes 0..5.
    WaveLds &wl = wlds[threadIdx.x >> 6];
    auto spmv = [&](const double (&qc)[kRowCache], auto &&tail) {
#pragma unroll
        for (int c = 0; c < kRowCache; ++c) wl.q[c][lane] = qc[c];
        wave_lds_sync();
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < kRowCache; ++c) {
            const double2 *qs = reinterpret_cast<const double2 *>(&wl.q[c][6 * (slot < 10 ? slot : 0)]);
            const double2 q01 = qs[0], q23 = qs[1], q45 = qs[2];
            if (cj[c] >= 0)
                acc += ((Bc[c][0] * q01.x + Bc[c][1] * q01.y) + (Bc[c][2] * q23.x + Bc[c][3] * q23.y)) + (Bc[c][4] * q45.x + Bc[c][5] * q45.y);
        }
        if (wide && slot < 10) {
            for (int b = beg + slot + 10 * kRowCache; b < end; b += 10) {
                const double *B = vals + 36 * (size_t)b + 6 * i;
                const size_t j6 = 6 * (size_t)col[b];
                const double q0 = tail(j6 + 0), q1 = tail(j6 + 1), q2 = tail(j6 + 2), q3 = tail(j6 + 3), q4 = tail(j6 + 4), q5 = tail(j6 + 5);
                acc += ((B[0] * q0 + B[1] * q1) + (B[2] * q2 + B[3] * q3)) + (B[4] * q4 + B[5] * q5);
            }
        }
        if (slot < 10) wl.part[i][slot] = acc;
        wave_lds_sync();
        const double2 *ps = reinterpret_cast<const double2 *>(&wl.part[lane < 6 ? lane : 0][0]);
        const double2 p01 = ps[0], p23 = ps[1], p45 = ps[2], p67 = ps[3], p89 = ps[4];
        return ((((((((p01.x + p01.y) + p23.x) + p23.y) + p45.x) + p45.y) + p67.x) + p67.y) + p89.x) + p89.y;
    };
    auto minv = [&](double v) {                                 // (M^-1 v)_lane from the six entries in lanes 0..5
        if (lane < 6) wl.w[lane] = v;
        wave_lds_sync();
        const double2 *ws = reinterpret_cast<const double2 *>(&wl.w[0]);
        const double2 w01 = ws[0], w23 = ws[1], w45 = ws[2];
        return ((((Mi[0] * w01.x + Mi[1] * w01.y) + Mi[2] * w23.x) + Mi[3] * w23.y) + Mi[4] * w45.x) + Mi[5] * w45.y;
    };
    // phase regions: u at +0, v at +N6, t at +2 N6 (pointer arithmetic, not a table of pointers: the accesses stay
    // global_load/global_store; a generic pointer's flat accesses would also count on lgkmcnt and stall the LDS barriers)
    auto region = [&](int k) { return ring + (size_t)(k & 3) * 3 * N6; };
    double xi = 0.0, ri = lead ? -rhs_i : 0.0, pi = 0.0, si = 0.0, ti = 0.0;
    double ui = minv(ri);
    if (lead) st_agent(region(0) + 6 * a + lane, nz_bits(ui));
    PRO_STAMP(4);
    request(region(0), false);
    await(region(0), false);
    PRO_STAMP(5);
    double wi = spmv(nu, [&](size_t j6) { return wait_for(region(0) + j6); });
    double vi = minv(wi);
    if (lead) {
        st_agent(region(0) + N6 + 6 * a + lane, nz_bits(vi));
        st_agent(region(0) + 2 * N6 + 6 * a + lane, -0.0);
    }
    if (!mine) ui = __builtin_nan("");
    double gamma = 0.0, delta = 0.0;
    double g = sum6_f64(lead ? ri * ui : 0.0), d = sum6_f64(lead ? wi * ui : 0.0);
    PRO_STAMP(6);
    double gamma_prev = 0.0, alpha_prev = 0.0;
#ifdef DFH_PCG_TRACE
    const int tw = (threadIdx.x >> 6) == (DFH_PCG_TRACE) && blockIdx.x < 64 ? (int)blockIdx.x : -1;
#endif
    for (int it = 0; it < iters; ++it) {
        const double *cur = region(it);
        const bool last = it == iters - 1;
        PCG_STAMP(0);
        grid_sum2(part + (size_t)it * 2 * nblk, ab, &lds, g, d, &gamma, &delta, !last, [&]() { request(cur, true); }, all_here, blk, nblk
#ifdef DFH_PCG_TRACE
                  , tw >= 0 && it < 16 ? &g_pcg_trace[tw][it][0] : nullptr
#endif
        );
        PCG_STAMP(1);
        const double beta = gamma_prev != 0.0 ? gamma / gamma_prev : 0.0;
        const double denom = alpha_prev != 0.0 ? delta - (beta * gamma) / alpha_prev : delta;
        const double alpha = denom != 0.0 ? gamma / denom : 0.0;
        if (lead) {
            pi = ui + beta * pi;
            si = wi + beta * si;
            ti = vi + beta * ti;
            xi += alpha * pi;
            ri = ri - alpha * si;
            ui = ui - alpha * ti;
        }
        if (last) break;
        PCG_STAMP(2);
        await(cur, true);
        PCG_STAMP(3);
        double qc[kRowCache];
#pragma unroll
        for (int c = 0; c < kRowCache; ++c) qc[c] = nu[c] - alpha * (nv[c] + beta * nt[c]);
        wi = spmv(qc, [&](size_t j6) { return wait_for(cur + j6) - alpha * (wait_for(cur + N6 + j6) + beta * wait_for(cur + 2 * N6 + j6)); });
        vi = minv(wi);
        double *nxt = region(it + 1);
        if (lead) {
            st_agent(nxt + 6 * a + lane, nz_bits(ui));
            st_agent(nxt + N6 + 6 * a + lane, nz_bits(vi));
            st_agent(nxt + 2 * N6 + 6 * a + lane, nz_bits(ti));
        }
        // region (it - 1) % 4: every reader was done with it before reduction `it`.  Cleared here, behind the publishing stores
        // (issued before the check of the neighbours' values, the clears' acknowledgements were waited for with the loads).
        if (it >= 1 && lead) {
            double *old = region(it - 1);
            st_agent(old + 6 * a + lane, 0.0);
            st_agent(old + N6 + 6 * a + lane, 0.0);
            st_agent(old + 2 * N6 + 6 * a + lane, 0.0);
        }
        if (!mine) ui = __builtin_nan("");
        g = sum6_f64(lead ? ri * ui : 0.0);
        d = sum6_f64(lead ? wi * ui : 0.0);
        PCG_STAMP(4);
        gamma_prev = gamma;
        alpha_prev = alpha;
    }
    if (!update_dq) {
        if (lead) x[6 * a + lane] = xi;
        return;
    }
    // The twist update is ALL OR NOTHING (round 4).  A time-out that falls into the last reduction leaves some workgroups with
    // finished rows and others with NaN; a wave applying its own row's step (round 3) then left node_dq half updated.  Now every
    // workgroup publishes its rows' x and takes a ticket (flag[2], zeroed with the scalars); the workgroup that draws the last
    // ticket knows that every other one is done, looks at the abort flag and at every row's x, and applies all N twists or none:
    // after a timed-out solve node_dq is what it was before the solve.
    if (lead) st_agent(x + 6 * a + lane, xi);
    __shared__ unsigned s_ticket;
    __syncthreads();                                                // (this workgroup's x stores are issued)
    if (threadIdx.x == 0)
        s_ticket = __hip_atomic_fetch_add(abort_flag + 2, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);   // release: after the x stores
    __syncthreads();
    if (s_ticket != (unsigned)nblk - 1u) return;
    bool bad = ab.raised();
    for (int r = (int)threadIdx.x; r < 6 * N; r += (int)blockDim.x) {
        const double v = ld_agent(x + r);
        bad = bad || !(fabs(v) < __builtin_huge_val());
    }
    if (__syncthreads_or(bad ? 1 : 0)) return;
    for (int r = (int)threadIdx.x; r < N; r += (int)blockDim.x) {
        const double *xr = x + 6 * (size_t)r;
        apply_twist_one(update_dq + 8 * (size_t)r, update_step * ld_agent(xr), update_step * ld_agent(xr + 1), update_step * ld_agent(xr + 2),
                        update_step * ld_agent(xr + 3), update_step * ld_agent(xr + 4), update_step * ld_agent(xr + 5));
    }
}

__global__ __launch_bounds__(256) void apply_twist_kernel(double *__restrict__ node_dq, const double *__restrict__ xi, int N,
                                                           double step) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= N) return;
    apply_twist_one(node_dq + 8 * a, step * xi[6 * a], step * xi[6 * a + 1], step * xi[6 * a + 2], step * xi[6 * a + 3],
                    step * xi[6 * a + 4], step * xi[6 * a + 5]);
}

// The multi-launch PCG's twist update, all or nothing like the persistent kernel's: x is final when this launch starts, so every
// workgroup looks at all 6N entries itself (same answer in each; no atomics, no host round trip) and applies its 256 twists only
// if every one is finite -- a NaN or an infinity in the system leaves node_dq as it was before the solve.
__global__ __launch_bounds__(256) void apply_twist_if_finite_kernel(double *__restrict__ node_dq, const double *__restrict__ xi, int N,
                                                                     double step) {
    bool bad = false;
    for (int r = (int)threadIdx.x; r < 6 * N; r += 256) bad = bad || !(fabs(xi[r]) < __builtin_huge_val());
    if (__syncthreads_or(bad ? 1 : 0)) return;
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= N) return;
    apply_twist_one(node_dq + 8 * (size_t)a, step * xi[6 * a], step * xi[6 * a + 1], step * xi[6 * a + 2], step * xi[6 * a + 3],
                    step * xi[6 * a + 4], step * xi[6 * a + 5]);
}

}  // namespace dfh

// ---- persistent-PCG bookkeeping ---------------------------------------------------------------------------------
// g_pcg_mode: 0 = auto (persistent kernel when co-residency holds, see pcg_solve_impl), 2 = always the two-launches-per-
// iteration path.  g_abort_count[dev]: device counter the persistent kernel bumps when a barrier times out.
// g_abort_host[dev]: a word of pinned host memory the kernel sets with the counter, so that the host can ask "anything
// timed out?" without a device call (dfh_pcg_status_peek).
namespace dfh { int g_pcg_mode = 0; unsigned long long *g_abort_count[64] = {nullptr}; unsigned *g_abort_host[64] = {nullptr}; }
using dfh::g_abort_count;
using dfh::g_abort_host;

static int pcg_abort_counter(unsigned long long **out) {
    int dev = 0;
    DFH_HIP_CHECK(hipGetDevice(&dev));
    DFH_REQUIRE(dev >= 0 && dev < 64, "device index %d out of range", dev);
    if (!g_abort_count[dev]) {
        unsigned long long *p = nullptr;
        DFH_HIP_CHECK(hipMalloc(reinterpret_cast<void **>(&p), sizeof(unsigned long long)));
        DFH_HIP_CHECK(hipMemset(p, 0, sizeof(unsigned long long)));
        unsigned *h = nullptr;
        if (hipHostMalloc(reinterpret_cast<void **>(&h), sizeof(unsigned), hipHostMallocMapped) == hipSuccess && h) {
            *h = 0u;
            g_abort_host[dev] = h;                          // (without it the peek always takes the synchronising path)
        } else {
            (void)hipGetLastError();
        }
        g_abort_count[dev] = p;
    }
    *out = g_abort_count[dev];
    return DFH_OK;
}

// Launch shape of a solve with n_nodes rows on the current device, and whether it takes the persistent kernel.
static int pcg_shape(int n_nodes, int *dev_out, int *wpb_out, int *nblk_out, bool *persistent_out) {
    using namespace dfh;
    int dev = 0;
    DFH_HIP_CHECK(hipGetDevice(&dev));
    DeviceInfo &di = device_info(dev);              // per DEVICE: a process may drive several
    if (di.n_cu == 0) DFH_HIP_CHECK(hipDeviceGetAttribute(&di.n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    const int n_cu = di.n_cu;
    // Workgroups of 8 waves (one row each) as long as they fit one per CU, of 16 beyond.  Measured at 2 048 rows (tools/kbench_pcg.py):
    // 256 workgroups x 8 waves 55 us per 10-iteration solve (slope 4.3 us, prologue 14.5), 128 x 16 waves 90 us (6.4 / 27.3).
    int wpb = (n_nodes + 7) / 8 <= n_cu ? 8 : 16;
    { const long v = opt().pcg_wpb; if (v == 4 || v == 8 || v == 16) wpb = (int)v; }
    const int nblk = (n_nodes + wpb - 1) / wpb;
    // Persistent path only when its grid barrier cannot starve: (1) the occupancy query says a workgroup of this size
    // fits on a CU, (2) the grid has at most one workgroup per CU (other kernels of this process may hold CUs for a while: they
    // end, the waiting workgroups then start; what must NOT run beside it is a second persistent solve that also wants most of
    // the chip -- two of them could wait for each other until the spin bound makes both leave and report DFH_E_TIMEOUT),
    // (3) the caller has not declared co-residency unsafe (dfh_pcg_set_mode(2): several processes time-sharing one GPU),
    // (4) the abort counter exists (it cannot be allocated while the stream is being captured: pcg_solve_impl).  Otherwise:
    // two launches per iteration, no spinning.
    bool persistent = nblk <= n_cu && nblk <= kMaxPcgBlocks && dfh::g_pcg_mode != 2 && !on(opt().pcg_multilaunch);
    if (persistent) {
        int &occ = wpb <= 8 ? di.pcg_occ512 : di.pcg_occ1024;
        if (occ < 0) {
            int nb = 0;
            const hipError_t e = wpb <= 8 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, pcg_cg1_kernel<512>, 64 * 8, 0)
                                          : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, pcg_cg1_kernel<1024>, 64 * 16, 0);
            occ = e == hipSuccess ? nb : 0;
        }
        persistent = occ >= 1;
    }
    *dev_out = dev; *wpb_out = wpb; *nblk_out = nblk; *persistent_out = persistent;
    return DFH_OK;
}

namespace dfh {

// the part of the workspace a solve expects all-zero at its start: the multi-launch path's first direction and its scalars, the
// persistent kernel's scalars, reduction slots and hand-off ring (zero bits = "not yet published")
void pcg_zero_range(void *workspace, int n_nodes, int iters, double **begin, size_t *count) {
    const size_t N6 = 6 * (size_t)n_nodes;
    const size_t n_scal = 3 * ((size_t)iters + 2) + 2 * ((size_t)iters + 1) * (((size_t)n_nodes + 3) / 4);
    *begin = static_cast<double *>(workspace) + 36 * (size_t)n_nodes + 4 * N6;         // = pA
    *count = N6 + n_scal + 12 * N6;
}

int pcg_solve_impl(const int *row_ptr, const int *col, double *vals, const double *rhs, int n_nodes, int iters,
                   double lm_abs, double lm_rel, double *x_out, void *workspace, size_t workspace_bytes, double *update_dq,
                   double update_step, void *stream, bool precleared) {
    DFH_REQUIRE(n_nodes >= 1 && iters >= 1, "dfh_pcg_solve: bad sizes");
    DFH_REQUIRE(row_ptr && col && vals && rhs && x_out && workspace, "dfh_pcg_solve: null pointer");
    DFH_REQUIRE(workspace_bytes >= dfh_pcg_workspace_bytes(n_nodes, iters), "dfh_pcg_solve: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    double *ws = static_cast<double *>(workspace);
    const size_t N6 = 6 * (size_t)n_nodes;
    double *Minv = ws; ws += 36 * (size_t)n_nodes;
    double *r = ws; ws += N6;
    double *Ap = ws; ws += N6;
    double *z = ws; ws += N6;
    double *pB = ws; ws += N6;
    double *pA = ws; ws += N6;                    // pA and the scalars are adjacent: one memset zeroes both
    double *scal = ws;                            // (beta = 0 in iteration 0 must not meet NaN garbage in pA)
    const size_t n_scal = 3 * ((size_t)iters + 2) + 2 * ((size_t)iters + 1) * (((size_t)n_nodes + 3) / 4);
    double *ring = scal + n_scal;                 // persistent kernel only; zero bits = "not yet published"
    PcgParams p{n_nodes, lm_abs, lm_rel};
    dim3 grid((n_nodes + 255) / 256), block(256);
    // One persistent launch when every row can have its own co-resident wave (pcg_shape: the decision, also behind dfh_pcg_path)
    int dev = 0, wpb = 8, nblk = 1;
    bool persistent = false;
    { const int rc = pcg_shape(n_nodes, &dev, &wpb, &nblk, &persistent); if (rc != DFH_OK) return rc; }
    // experiment (option pcg_one_xcd = the stride, 8 on MI355X): every working workgroup on one die, 16-wave workgroups so that
    // up to 1 024 rows fit its 32 CUs two per CU.  Measured (profiles/r4_pcg_one_xcd.txt) -- not the default.
    int die_stride = 1;
    if (persistent && opt().pcg_one_xcd > 1 && n_nodes <= 1024) {
        die_stride = (int)opt().pcg_one_xcd;
        wpb = 16;
        nblk = (n_nodes + wpb - 1) / wpb;
    }
    unsigned long long *abort_count = nullptr;
    if (persistent) {
        if (dev >= 0 && dev < 64 && g_abort_count[dev]) {
            abort_count = g_abort_count[dev];
        } else {
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(s, &cs) != hipSuccess) cs = hipStreamCaptureStatusNone;
            if (cs == hipStreamCaptureStatusNone) {
                const int rc = pcg_abort_counter(&abort_count);
                if (rc != DFH_OK) return rc;
            } else {
                persistent = false;
            }
        }
    }
    unsigned *abort_host = nullptr;
    if (persistent) {
        if (dev >= 0 && dev < 64 && g_abort_host[dev] &&
            hipHostGetDevicePointer(reinterpret_cast<void **>(&abort_host), g_abort_host[dev], 0) != hipSuccess) {
            (void)hipGetLastError();
            abort_host = nullptr;
        }
        if (!precleared) DFH_HIP_CHECK(hipMemsetAsync(scal, 0, sizeof(double) * (n_scal + 12 * N6), s));
        unsigned spin_limit = kSpinLimit;
        if (opt().pcg_spin_limit >= 0) spin_limit = (unsigned)opt().pcg_spin_limit;
        unsigned *flag = reinterpret_cast<unsigned *>(scal + 3 * ((size_t)iters + 1));    // spare scalar: abort flag
        double *part = scal + 3 * ((size_t)iters + 2);                                    // (2 per iteration + 1) reductions x nblk slots
        if (wpb <= 8)
            hipLaunchKernelGGL(pcg_cg1_kernel<512>, dim3(nblk * die_stride), dim3(64 * wpb), 0, s, row_ptr, col, vals, rhs, p, iters, x_out, ring, part,
                               flag, spin_limit, abort_count, abort_host, update_dq, update_step, die_stride);
        else
            hipLaunchKernelGGL(pcg_cg1_kernel<1024>, dim3(nblk * die_stride), dim3(64 * wpb), 0, s, row_ptr, col, vals, rhs, p, iters, x_out, ring, part,
                               flag, spin_limit, abort_count, abort_host, update_dq, update_step, die_stride);
        DFH_HIP_CHECK(hipGetLastError());
        return DFH_OK;
    }
    if (!precleared) DFH_HIP_CHECK(hipMemsetAsync(pA, 0, sizeof(double) * (N6 + n_scal), s));
    // dot products: per-workgroup partials in the slots the persistent kernel uses for its reductions (2 (iters + 1) slots of
    // ceil(N / 4) doubles): slot 2 it = p.Ap of iteration it, 2 it + 1 = r.z after it, slot 2 iters = r.z of the init
    const size_t nq = ((size_t)n_nodes + 3) / 4;
    double *part = scal + 3 * ((size_t)iters + 2);
    const int n_init = (int)grid.x, n_spmv = (n_nodes + 3) / 4, n_upd = (n_nodes + 39) / 40;
    hipLaunchKernelGGL(pcg_init_kernel, grid, block, 0, s, row_ptr, col, vals, rhs, p, Minv, x_out, r, z, part + 2 * (size_t)iters * nq);
    double *p_prev = pA, *p_cur = pB;
    for (int it = 0; it < iters; ++it) {
        double *sc = scal + 3 * ((size_t)it + 1);
        // iteration 0: the scalars in front of sc are zero (cleared above): rz_prev = 0 gives beta = 0
        const double *rz_part = it == 0 ? part + 2 * (size_t)iters * nq : part + (2 * (size_t)it - 1) * nq;
        hipLaunchKernelGGL(pcg_spmv_kernel, dim3(n_spmv), block, 0, s, row_ptr, col, vals, n_nodes, z, p_prev, p_cur,
                           Ap, sc - 3, sc, rz_part, it == 0 ? n_init : n_upd, part + 2 * (size_t)it * nq);
        hipLaunchKernelGGL(pcg_update_xr_kernel, dim3(n_upd), block, 0, s, n_nodes, Minv, x_out, r, p_cur, Ap, z, sc,
                           part + 2 * (size_t)it * nq, n_spmv, part + (2 * (size_t)it + 1) * nq);
        double *t = p_prev; p_prev = p_cur; p_cur = t;
    }
    if (update_dq)
        hipLaunchKernelGGL(apply_twist_if_finite_kernel, dim3((n_nodes + 255) / 256), dim3(256), 0, s, update_dq, x_out, n_nodes, update_step);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

}  // namespace dfh

// =================================================================================== C ABI
extern "C" {

size_t dfh_pcg_workspace_bytes(int n_nodes, int iters) {
    if (n_nodes <= 0 || iters < 0) return 0;
    // Minv (36N) + r,pA,Ap,z,pB (5*6N) + scalars (3 per iteration + 6) + per-workgroup partial sums + the persistent
    // kernel's ring of published vectors (4 x 3 x 6N)
    return sizeof(double) * ((size_t)36 * n_nodes + (size_t)30 * n_nodes + 3 * ((size_t)iters + 2) +
                             2 * ((size_t)iters + 1) * (((size_t)n_nodes + 3) / 4) + (size_t)72 * n_nodes);
}

int dfh_pcg_set_mode(int mode) {
    DFH_REQUIRE(mode == 0 || mode == 2, "dfh_pcg_set_mode: mode %d (0 = auto, 2 = multi-launch)", mode);
    dfh::g_pcg_mode = mode;
    return DFH_OK;
}

int dfh_pcg_status(void *stream, long *aborted_solves_out) {
    using namespace dfh;
    DFH_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    int dev = 0;
    DFH_HIP_CHECK(hipGetDevice(&dev));
    unsigned long long n = 0;
    if (dev >= 0 && dev < 64 && g_abort_count[dev]) {
        DFH_HIP_CHECK(hipMemcpy(&n, g_abort_count[dev], sizeof(n), hipMemcpyDeviceToHost));
        if (n) DFH_HIP_CHECK(hipMemset(g_abort_count[dev], 0, sizeof(n)));
        if (g_abort_host[dev]) *g_abort_host[dev] = 0u;
    }
    if (aborted_solves_out) *aborted_solves_out = (long)n;
    if (n)
        return fail(DFH_E_TIMEOUT, "persistent PCG: %llu solve(s) timed out in a grid barrier (workgroups not co-resident?); x = NaN; "
                                   "a timed-out solve leaves node_dq as it was before that solve (the twist update is all or nothing)", n);
    return DFH_OK;
}

int dfh_pcg_status_peek(void *stream, long *aborted_solves_out) {
    using namespace dfh;
    int dev = 0;
    DFH_HIP_CHECK(hipGetDevice(&dev));
    if (dev >= 0 && dev < 64 && (!g_abort_count[dev] || (g_abort_host[dev] && *static_cast<volatile unsigned *>(g_abort_host[dev]) == 0u))) {
        if (aborted_solves_out) *aborted_solves_out = 0;    // no persistent solve yet, or none that has completed timed out
        return DFH_OK;
    }
    return dfh_pcg_status(stream, aborted_solves_out);
}

int dfh_pcg_path(int n_nodes) {
    DFH_REQUIRE(n_nodes >= 1, "dfh_pcg_path: bad node count");
    int dev = 0, wpb = 0, nblk = 0;
    bool persistent = false;
    const int rc = pcg_shape(n_nodes, &dev, &wpb, &nblk, &persistent);
    if (rc != DFH_OK) return rc;
    return persistent ? 1 : 2;
}

#ifdef DFH_PCG_TRACE
int dfh_debug_pcg_trace(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(dfh::g_pcg_trace), sizeof(unsigned long long) * 64 * 16 * 12) == hipSuccess ? 0 : -1;
}
#endif

int dfh_pcg_solve(const int *row_ptr, const int *col, double *vals, const double *rhs, int n_nodes, int iters,
                  double lm_abs, double lm_rel, double *x_out, void *workspace, size_t workspace_bytes, void *stream) {
    return dfh::pcg_solve_impl(row_ptr, col, vals, rhs, n_nodes, iters, lm_abs, lm_rel, x_out, workspace, workspace_bytes, nullptr, 0.0, stream);
}

int dfh_pcg_solve_update(const int *row_ptr, const int *col, double *vals, const double *rhs, int n_nodes, int iters,
                         double lm_abs, double lm_rel, double *x_out, void *workspace, size_t workspace_bytes, double *node_dq,
                         double step, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(node_dq, "dfh_pcg_solve_update: null node_dq");
    return pcg_solve_impl(row_ptr, col, vals, rhs, n_nodes, iters, lm_abs, lm_rel, x_out, workspace, workspace_bytes, node_dq, step, stream);
}

int dfh_apply_twist(double *node_dq, const double *xi, int n_nodes, double step, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(n_nodes >= 0, "dfh_apply_twist: negative count");
    if (n_nodes == 0) return DFH_OK;
    DFH_REQUIRE(node_dq && xi, "dfh_apply_twist: null pointer");
    hipLaunchKernelGGL(apply_twist_kernel, dim3((n_nodes + 255) / 256), dim3(256), 0, (hipStream_t)stream, node_dq, xi, n_nodes, step);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

}  // extern "C"
