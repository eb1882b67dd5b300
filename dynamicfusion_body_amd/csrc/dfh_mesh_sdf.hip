// K22  mesh -> signed distance: the exact distance from points (or the vertices of a regular grid) to a triangle mesh, with the
// closest point, the winning face and an angle-weighted-pseudonormal sign (dfh_mesh_sdf_*).  No reference counterpart: the
// reference reads `.dist` files, this makes what goes inside.  The result is written out operation by operation in
// include/dfusion_hip.h; tests/mesh_sdf_np.py restates it by brute force over all faces and agrees bit for bit.
//
// Shape.  A uniform cell table over the mesh's box (count -> scan -> fill, the scan being dfh_scan.h's; every kept face is
// listed in every cell its box overlaps, each entry with its cell's z index).  One wave (= one workgroup) owns 64 query
// points: a 4 x 4 x 4 block of grid vertices or 64 consecutive points.  It walks the cells around its block shell by shell; the lanes read the entries of a run of
// cells, keep each face once (below), stage the kept faces' nine coordinates in LDS (kMsdChunk faces: 4.75 KB a wave) and then
// every lane evaluates every staged face (one IEEE division a face: the region is chosen first, then ONE quotient is formed).
// The winner is a minimum over a set under a total order (d2, then face index), so neither the order of the entries in a cell
// (integer atomics in the fill) nor the order of the cells can change a bit.  No float atomics, no private arrays, no scratch.
//
// Cells.  b_a(k) = lo_a + (double)k * h, as computed (product, then sum), is non-decreasing in k.  cell_a(x) is the largest
// k in [0, n_a - 1] with b_a(k) <= x, and 0 if there is none (msd_cell: an estimate from (x - lo) / h, then corrected against
// b_a itself, so the definition does not depend on the estimate's rounding).  Hence for 1 <= k <= n_a - 1:
//     cell_a(x) <  k  <=>  x <  b_a(k)          (*)
// A kept face with per-axis coordinate range [fmin_a, fmax_a] is listed in every cell of [cell(fmin), cell(fmax)] (its range).
//
// Each face once.  After shell r the visited cells are the box R = [R0, R1], R0 = max(clo - r, 0), R1 = min(chi + r, n - 1) with
// clo = cell(block's min corner), chi = cell(block's max corner); the shell is R minus the previous box.  A face whose range
// meets the previous box was evaluated in an earlier shell.  A face that meets R but not the previous box is taken from exactly
// one of its entries, the one in cell max(f0, R0) (componentwise): that cell lies in the face's range and in R, and, the range
// missing the previous box, in the shell.
//
// Stopping rule.  Claim: after shell r, every face not yet evaluated has a COMPUTED d2 > L2(lane), with
//     D  = min over the axes a of  { P_a - b_a(R0_a)  if R0_a >= 1;   b_a(R1_a + 1) - P_a  if R1_a <= n_a - 2 },
//     s  = D (1 - 2^-48) - delta,       L2 = s > 0 ? (s s)(1 - 2^-48) : 0,      delta = 2^-40 max|vertex coordinate|.
// Proof.  An unevaluated face's range misses R on some axis a.  Either cell(fmax_a) < R0_a, so R0_a >= 1 and by (*)
// fmax_a < b_a(R0_a); every lane has cell(P_a) >= clo_a >= R0_a >= 1, so P_a >= b_a(R0_a), and every point X of the triangle has
// P_a - X_a > P_a - b_a(R0_a) >= 0.  Or cell(fmin_a) > R1_a, so R1_a + 1 <= n_a - 1 and fmin_a >= b_a(R1_a + 1), while
// cell(P_a) <= chi_a <= R1_a < n_a - 1 gives P_a < b_a(R1_a + 1) by (*): X_a - P_a > b_a(R1_a + 1) - P_a > 0.  So the true
// distance from P to the triangle exceeds the exact value of D's winning term.  Rounding, all directions downward: the
// computed difference is within 2^-53 relative of the exact one, and the factor (1 - 2^-48) more than covers it, so
// D (1 - 2^-48) is below the true distance.  The computed closest point Q' lies within delta' <= 2^-48 max|coordinate| of a point
// of the triangle (a vertex is exact; an edge point is A + t ab with t in [0, 1] as computed, two roundings of magnitudes
// <= 3 max|coordinate|; the face point two more; this assumes region 7's computed weights stay in [-1, 2], which fails only for
// slivers whose va + vb + vc cancels to nothing -- such a face's Q' is not bounded by this proof), so |P - Q'| > s + (delta -
// delta') with delta = 256 delta', and the computed d2 = |P - Q'|^2 carries at most 2^-50 relative error: d2 > (s s)(1 - 2^-48)
// >= L2 as computed (the products round within 2^-52).  A lane stops when best < L2, STRICTLY (so no unvisited face can even
// tie and win on its index; L2 = 0 never stops), or when band^2 < L2 (everything unvisited is far: if best > band^2 too the point
// is far, else best < L2 already).  The wave stops when all its lanes do, or when R is the whole table.
// The same bound with the two boxes (block, mesh) in place of (point, shell) lets a block farther than band skip the search.
#include <climits>
#include <cmath>

#include "dfh_common.h"
#include "dfh_scan.h"

namespace dfh {

constexpr int kMsdChunk = 64;           // faces staged in LDS between two evaluation passes (dfh_mesh_sdf_chunk)
constexpr int kMsdMaxDim = 128;         // cells per axis at most (the packed ranges hold 10 bits an axis)
constexpr double kMsdShrink = 1.0 - 0x1p-48;

__host__ __device__ __forceinline__ double msd_bound(double lo, double h, int k) { return lo + (double)k * h; }

// cell(x) of the header: the largest k in [0, n-1] with b(k) <= x, 0 if none (a NaN gives 0)
__host__ __device__ __forceinline__ int msd_cell(double x, double lo, double h, double inv_h, int n) {
    const double t = (x - lo) * inv_h;
    int c = !(t > 0.0) ? 0 : (t >= (double)(n - 1) ? n - 1 : (int)t);
    while (c + 1 < n && msd_bound(lo, h, c + 1) <= x) ++c;
    while (c > 0 && msd_bound(lo, h, c) > x) --c;
    return c;
}

struct MsdTable {                        // the cell table's geometry and its arrays inside the caller's buffer
    double lo[3], hi[3], h, inv_h, delta;
    int n[3];
    long n_faces, n_entries;
    int *cell_start;                     // ncells + 1
    int *cursor;                         // ncells
    uint2 *frange;                       // n_faces: packed (lo, hi) cell ranges
    int2 *entries;                       // n_entries: (face, cell z)
};

static size_t msd_align8(size_t b) { return (b + 7) & ~(size_t)7; }

static size_t msd_table_bytes(const int n[3], long n_faces, long n_entries) {
    const size_t nc = (size_t)n[0] * n[1] * n[2];
    return msd_align8((nc + 1) * 4) + msd_align8(nc * 4) + (size_t)n_faces * 8 + (size_t)n_entries * 8;
}

__host__ __device__ __forceinline__ unsigned msd_pack(int x, int y, int z) { return (unsigned)x | ((unsigned)y << 10) | ((unsigned)z << 20); }

// ---- the table: count -> scan -> fill -------------------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(256) void msd_bin_kernel(MsdTable t, const double *__restrict__ verts, const int *__restrict__ faces,
                                                      const unsigned char *__restrict__ keep) {
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f >= t.n_faces) return;
    if (!keep[f]) {
        if (!FILL) t.frange[f] = make_uint2(msd_pack(1, 1, 1), msd_pack(0, 0, 0));
        return;
    }
    int c0[3], c1[3];
    const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double xa = verts[3 * (long)ia + a], xb = verts[3 * (long)ib + a], xc = verts[3 * (long)ic + a];
        c0[a] = msd_cell(fmin(xa, fmin(xb, xc)), t.lo[a], t.h, t.inv_h, t.n[a]);
        c1[a] = msd_cell(fmax(xa, fmax(xb, xc)), t.lo[a], t.h, t.inv_h, t.n[a]);
    }
    if (!FILL) t.frange[f] = make_uint2(msd_pack(c0[0], c0[1], c0[2]), msd_pack(c1[0], c1[1], c1[2]));
    for (int x = c0[0]; x <= c1[0]; ++x)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int z = c0[2]; z <= c1[2]; ++z) {
                const long c = ((long)x * t.n[1] + y) * t.n[2] + z;
                const int pos = atomicAdd(&t.cursor[c], 1);
                if (FILL && pos < t.cell_start[c + 1] && pos < t.n_entries) t.entries[pos] = make_int2((int)f, z);
            }
}

// exclusive scan of cursor[0..nc) into cell_start[0..nc] and back into cursor (one workgroup: the table has at most 2^21 cells,
// 256 rounds of dfh_scan.h's block_scan_rounds at eight cells a thread)
__global__ __launch_bounds__(1024) void msd_scan_kernel(MsdTable t, long nc) {
    __shared__ int wtot[16];
    const int sum = block_scan_rounds<16, 8, int>(
        nc, wtot, [&](long i) { return t.cursor[i]; }, [&](long i, int at) { t.cell_start[i] = at; t.cursor[i] = at; });
    if (threadIdx.x == 0) t.cell_start[nc] = sum;
}

// ---- the query ------------------------------------------------------------------------------------------------------------
struct MsdQuery {
    MsdTable t;
    const double *verts;
    const int *faces;
    const double *fn, *en, *vn;          // face (F,3), edge (F,3,3), vertex (Nv,3) pseudonormals
    double band, band2, orient;
    long n_waves;
    // points
    const double *points;
    long n_points;
    // grid
    double origin[3], spacing[3];
    int X, Y, Z, nbx, nby, nbz;
    // outputs
    void *value;                          // points: double; grid: VT
    signed char *status;                  // grid with a finite band: 0 far, 1 known >= 0, 2 known < 0
    float *closest;
    int *face;
};

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmin(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

struct MsdBest {
    double d2, qx, qy, qz;
    int f, feat;
};

// every lane against the n staged faces (the region walk of the header; one division per face)
__device__ __forceinline__ void msd_evaluate(const double *__restrict__ sv, const int *__restrict__ sf, int n, double px, double py, double pz,
                                             MsdBest &b) {
    for (int j = 0; j < n; ++j) {
        const double *v = sv + 9 * j;
        const double ax = v[0], ay = v[1], az = v[2], bx = v[3], by = v[4], bz = v[5], cx = v[6], cy = v[7], cz = v[8];
        const int f = sf[j];
        const double abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
        const double apx = px - ax, apy = py - ay, apz = pz - az;
        const double d1 = (abx * apx + aby * apy) + abz * apz, d2 = (acx * apx + acy * apy) + acz * apz;
        const double bpx = px - bx, bpy = py - by, bpz = pz - bz;
        const double d3 = (abx * bpx + aby * bpy) + abz * bpz, d4 = (acx * bpx + acy * bpy) + acz * bpz;
        const double cpx = px - cx, cpy = py - cy, cpz = pz - cz;
        const double d5 = (abx * cpx + aby * cpy) + abz * cpz, d6 = (acx * cpx + acy * cpy) + acz * cpz;
        const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
        const double e43 = d4 - d3, e56 = d5 - d6;
        int feat;
        if (d1 <= 0.0 && d2 <= 0.0) feat = 0;
        else if (d3 >= 0.0 && d4 <= d3) feat = 1;
        else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) feat = 3;
        else if (d6 >= 0.0 && d5 <= d6) feat = 2;
        else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) feat = 4;
        else if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) feat = 5;
        else feat = 6;
        const double num = feat == 3 ? d1 : feat == 4 ? d2 : feat == 5 ? e43 : 1.0;
        const double den = feat == 3 ? d1 - d3 : feat == 4 ? d2 - d6 : feat == 5 ? e43 + e56 : (va + vb) + vc;
        const double q = num / den;                                        // the edge parameter, or 1 / (va + vb + vc)
        // base + t1 e1 (+ t2 ac on the face)
        const bool fromB = feat == 5;
        const double ox = fromB ? bx : ax, oy = fromB ? by : ay, oz = fromB ? bz : az;
        const double ex = feat == 4 ? acx : feat == 5 ? cx - bx : abx, ey = feat == 4 ? acy : feat == 5 ? cy - by : aby,
                     ez = feat == 4 ? acz : feat == 5 ? cz - bz : abz;
        const double t1 = feat == 6 ? vb * q : q;
        double qx = ox + t1 * ex, qy = oy + t1 * ey, qz = oz + t1 * ez;
        if (feat == 6) {
            const double t2 = vc * q;
            qx = qx + t2 * acx; qy = qy + t2 * acy; qz = qz + t2 * acz;
        }
        if (feat == 0) { qx = ax; qy = ay; qz = az; }
        if (feat == 1) { qx = bx; qy = by; qz = bz; }
        if (feat == 2) { qx = cx; qy = cy; qz = cz; }
        const double dx = px - qx, dy = py - qy, dz = pz - qz;
        const double dd = (dx * dx + dy * dy) + dz * dz;
        if (dd < b.d2 || (dd == b.d2 && f < b.f)) {
            b.d2 = dd; b.qx = qx; b.qy = qy; b.qz = qz; b.f = f; b.feat = feat;
        }
    }
}

template <typename VT, bool GRID>
__global__ __launch_bounds__(64) void msd_query_kernel(MsdQuery a) {
    __shared__ double sv[kMsdChunk * 9];
    __shared__ int sf[kMsdChunk];
    const int lane = threadIdx.x;
    const long wave = blockIdx.x;
    const MsdTable &t = a.t;

    bool valid;
    double px, py, pz;
    long out;
    if (GRID) {
        const int wz = (int)(wave % a.nbz), wy = (int)((wave / a.nbz) % a.nby), wx = (int)(wave / ((long)a.nbz * a.nby));
        const int i = wx * 4 + (lane >> 4), j = wy * 4 + ((lane >> 2) & 3), k = wz * 4 + (lane & 3);
        valid = i < a.X && j < a.Y && k < a.Z;
        px = a.origin[0] + (double)i * a.spacing[0];
        py = a.origin[1] + (double)j * a.spacing[1];
        pz = a.origin[2] + (double)k * a.spacing[2];
        out = ((long)i * a.Y + j) * a.Z + k;
    } else {
        out = wave * 64 + lane;
        valid = out < a.n_points;
        px = valid ? a.points[3 * out] : 0.0;
        py = valid ? a.points[3 * out + 1] : 0.0;
        pz = valid ? a.points[3 * out + 2] : 0.0;
    }
    const double p[3] = {px, py, pz};     // (indexed by unrolled constants only)
    double bmin[3], bmax[3];
    int clo[3], chi[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        bmin[x] = wave_min(valid ? p[x] : INFINITY);
        bmax[x] = wave_max(valid ? p[x] : -INFINITY);
        clo[x] = msd_cell(bmin[x], t.lo[x], t.h, t.inv_h, t.n[x]);
        chi[x] = msd_cell(bmax[x], t.lo[x], t.h, t.inv_h, t.n[x]);
    }
    // a block farther than band from the mesh's box: every point is far, no search
    bool search = true;
    if (a.band2 < INFINITY) {
        double gg = 0.0;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const double g = fmax(fmax(t.lo[x] - bmax[x], bmin[x] - t.hi[x]), 0.0);
            gg += g * g;
        }
        const double s = sqrt(gg) * kMsdShrink - t.delta;
        if (s > 0.0 && (s * s) * kMsdShrink > a.band2) search = false;
    }

    MsdBest b;
    b.d2 = INFINITY; b.qx = b.qy = b.qz = 0.0; b.f = INT_MAX; b.feat = 6;
    int nst = 0;
    for (int r = 0; search; ++r) {
        int R0[3], R1[3], P0[3], P1[3];
        bool covered = true;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            R0[x] = max(clo[x] - r, 0);
            R1[x] = min(chi[x] + r, t.n[x] - 1);
            P0[x] = r > 0 ? max(clo[x] - (r - 1), 0) : 1;
            P1[x] = r > 0 ? min(chi[x] + (r - 1), t.n[x] - 1) : 0;
            covered = covered && R0[x] == 0 && R1[x] == t.n[x] - 1;
        }
        for (int cx = R0[0]; cx <= R1[0]; ++cx)
            for (int cy = R0[1]; cy <= R1[1]; ++cy) {
                const bool inxy = r > 0 && cx >= P0[0] && cx <= P1[0] && cy >= P0[1] && cy <= P1[1];
                const long base = ((long)cx * t.n[1] + cy) * t.n[2];
                for (int seg = 0; seg < (inxy ? 2 : 1); ++seg) {
                    const int za = !inxy ? R0[2] : seg == 0 ? R0[2] : P1[2] + 1;
                    const int zb = !inxy ? R1[2] : seg == 0 ? P0[2] - 1 : R1[2];
                    if (za > zb) continue;
                    const int e1 = t.cell_start[base + zb + 1];
                    for (int e = t.cell_start[base + za]; e < e1;) {
                        const int take = min(kMsdChunk - nst, e1 - e);
                        bool keep = false;
                        int f = 0;
                        if (lane < take) {
                            const int2 ent = t.entries[e + lane];
                            f = ent.x;
                            const uint2 rg = t.frange[f];
                            const int f0x = rg.x & 1023, f0y = (rg.x >> 10) & 1023, f0z = (rg.x >> 20) & 1023;
                            const int f1x = rg.y & 1023, f1y = (rg.y >> 10) & 1023, f1z = (rg.y >> 20) & 1023;
                            const bool meets_prev = r > 0 && f1x >= P0[0] && f0x <= P1[0] && f1y >= P0[1] && f0y <= P1[1] && f1z >= P0[2] && f0z <= P1[2];
                            keep = !meets_prev && cx == max(f0x, R0[0]) && cy == max(f0y, R0[1]) && ent.y == max(f0z, R0[2]);
                        }
                        const unsigned long long mask = __ballot(keep);
                        if (keep) {
                            const int pos = nst + __popcll(mask & ((1ull << lane) - 1ull));
                            sf[pos] = f;
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                const long vi = a.faces[3 * (long)f + c];
                                sv[9 * pos + 3 * c] = a.verts[3 * vi];
                                sv[9 * pos + 3 * c + 1] = a.verts[3 * vi + 1];
                                sv[9 * pos + 3 * c + 2] = a.verts[3 * vi + 2];
                            }
                        }
                        nst += __popcll(mask);
                        e += take;
                        if (nst == kMsdChunk) {
                            __syncthreads();
                            msd_evaluate(sv, sf, nst, px, py, pz, b);
                            __syncthreads();
                            nst = 0;
                        }
                    }
                }
            }
        if (nst) {
            __syncthreads();
            msd_evaluate(sv, sf, nst, px, py, pz, b);
            __syncthreads();
            nst = 0;
        }
        if (covered) break;
        double D = INFINITY;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            if (R0[x] >= 1) D = fmin(D, p[x] - msd_bound(t.lo[x], t.h, R0[x]));
            if (R1[x] <= t.n[x] - 2) D = fmin(D, msd_bound(t.lo[x], t.h, R1[x] + 1) - p[x]);
        }
        const double s = D * kMsdShrink - t.delta;
        const double L2 = s > 0.0 ? (s * s) * kMsdShrink : 0.0;
        const bool done = !valid || b.d2 < L2 || a.band2 < L2;
        if (__all(done)) break;
    }
    if (!valid) return;

    const bool known = b.f != INT_MAX && b.d2 <= a.band2;
    double val = a.band;
    bool neg = false;
    if (known) {
        const double *N = b.feat == 6 ? a.fn + 3 * (long)b.f
                          : b.feat >= 3 ? a.en + 3 * (3 * (long)b.f + (b.feat - 3))
                                        : a.vn + 3 * (long)a.faces[3 * (long)b.f + b.feat];
        const double dot = ((px - b.qx) * N[0] + (py - b.qy) * N[1]) + (pz - b.qz) * N[2];
        neg = dot * a.orient < 0.0 && b.d2 != 0.0;
        val = sqrt(b.d2);
        val = b.d2 == 0.0 ? 0.0 : neg ? -val : val;
    }
    ((VT *)a.value)[out] = (VT)val;
    if (a.status) a.status[out] = known ? (neg ? 2 : 1) : 0;
    if (a.closest) {
        const float nanf_ = __builtin_nanf("");
        a.closest[3 * out] = known ? (float)b.qx : nanf_;
        a.closest[3 * out + 1] = known ? (float)b.qy : nanf_;
        a.closest[3 * out + 2] = known ? (float)b.qz : nanf_;
    }
    if (a.face) a.face[out] = known ? b.f : -1;
}

// ---- far fill: one thread per line of the axis; status 0 undecided, 1 / 2 known (+ / -), 3 / 4 filled (+ / -) -----------------
// AXIS 2 = z (the first sweep), 1 = y, 0 = x (the last: a line still undecided becomes +).
template <typename VT, int AXIS>
__global__ __launch_bounds__(256) void msd_fill_kernel(VT *__restrict__ value, signed char *__restrict__ st, int X, int Y, int Z, double band) {
    const long nlines = AXIS == 2 ? (long)X * Y : AXIS == 1 ? (long)X * Z : (long)Y * Z;
    const long l = (long)blockIdx.x * 256 + threadIdx.x;
    if (l >= nlines) return;
    const int L = AXIS == 2 ? Z : AXIS == 1 ? Y : X;
    const long stride = AXIS == 2 ? 1 : AXIS == 1 ? Z : (long)Y * Z;
    const long base = AXIS == 2 ? l * Z : AXIS == 1 ? (l / Z) * ((long)Y * Z) + l % Z : l;
    int first = 0;
    for (int i = 0; i < L && !first; ++i) first = st[base + i * stride];
    if (!first && AXIS != 0) return;
    bool neg = first == 2 || first == 4;
    const VT pos_v = (VT)band, neg_v = (VT)(-band);
    for (int i = 0; i < L; ++i) {
        const long o = base + i * stride;
        const int s = st[o];
        if (s) neg = s == 2 || s == 4;
        else {
            st[o] = neg ? 4 : 3;
            value[o] = neg ? neg_v : pos_v;
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static int msd_check_mesh(const char *what, const dfh_mesh_sdf *m) {
    DFH_REQUIRE(m, "%s: null mesh", what);
    DFH_REQUIRE(m->verts && m->faces && m->keep && m->face_normals && m->edge_normals && m->vertex_normals, "%s: null mesh array", what);
    DFH_REQUIRE(m->table, "%s: null table", what);
    const dfh_mesh_sdf_layout &l = m->layout;
    DFH_REQUIRE(m->n_verts > 0 && m->n_faces > 0 && m->n_faces < (1l << 31) && m->n_verts < (1l << 31), "%s: bad mesh size", what);
    DFH_REQUIRE(l.n_faces == m->n_faces && l.n_verts == m->n_verts, "%s: the layout is of another mesh", what);
    DFH_REQUIRE(l.cell > 0.0 && std::isfinite(l.cell) && std::isfinite(l.maxabs) && l.maxabs >= 0.0, "%s: bad layout", what);
    for (int a = 0; a < 3; ++a) {
        DFH_REQUIRE(l.dims[a] >= 1 && l.dims[a] <= kMsdMaxDim, "%s: bad layout dims", what);
        DFH_REQUIRE(std::isfinite(l.lo[a]) && std::isfinite(l.hi[a]) && l.lo[a] <= l.hi[a], "%s: bad layout box", what);
    }
    DFH_REQUIRE(l.n_entries > 0 && l.n_entries < (1l << 31), "%s: bad layout entry count", what);
    DFH_REQUIRE(l.bytes == msd_table_bytes(l.dims, l.n_faces, l.n_entries) && m->table_bytes >= l.bytes, "%s: table too small", what);
    return DFH_OK;
}

static MsdTable msd_table(const dfh_mesh_sdf *m) {
    const dfh_mesh_sdf_layout &l = m->layout;
    MsdTable t;
    for (int a = 0; a < 3; ++a) { t.lo[a] = l.lo[a]; t.hi[a] = l.hi[a]; t.n[a] = l.dims[a]; }
    t.h = l.cell;
    t.inv_h = 1.0 / l.cell;
    t.delta = 0x1p-40 * l.maxabs;
    t.n_faces = l.n_faces;
    t.n_entries = l.n_entries;
    const size_t nc = (size_t)l.dims[0] * l.dims[1] * l.dims[2];
    char *p = (char *)m->table;
    t.cell_start = (int *)p; p += msd_align8((nc + 1) * 4);
    t.cursor = (int *)p;     p += msd_align8(nc * 4);
    t.frange = (uint2 *)p;   p += (size_t)l.n_faces * 8;
    t.entries = (int2 *)p;
    return t;
}

static int msd_check_band(const char *what, double band, int orientation) {
    DFH_REQUIRE(band > 0.0, "%s: band must be > 0 (or +inf), got %g", what, band);   // (a NaN fails)
    DFH_REQUIRE(orientation == 1 || orientation == -1, "%s: orientation must be +1 or -1, got %d", what, orientation);
    return DFH_OK;
}

static void msd_query_common(MsdQuery &q, const dfh_mesh_sdf *m, double band, int orientation) {
    q.t = msd_table(m);
    q.verts = m->verts; q.faces = m->faces;
    q.fn = m->face_normals; q.en = m->edge_normals; q.vn = m->vertex_normals;
    q.band = band; q.band2 = band * band; q.orient = (double)orientation;
}

}  // namespace dfh

using namespace dfh;

extern "C" int dfh_mesh_sdf_chunk(void) { return kMsdChunk; }

extern "C" int dfh_mesh_sdf_plan(const double *verts, long n_verts, const int *faces, const unsigned char *keep, long n_faces, double cell,
                                 dfh_mesh_sdf_layout *out) {
    const char *what = "dfh_mesh_sdf_plan";
    DFH_REQUIRE(verts && faces && keep && out, "%s: null argument", what);
    DFH_REQUIRE(n_faces > 0, "%s: a mesh without faces (F == 0)", what);
    DFH_REQUIRE(n_verts > 0 && n_verts < (1l << 31) && n_faces < (1l << 31), "%s: bad mesh size", what);
    DFH_REQUIRE(cell >= 0.0 && std::isfinite(cell), "%s: cell must be finite and >= 0 (0: chosen here), got %g", what, cell);
    double maxabs = 0.0;
    for (long i = 0; i < 3 * n_verts; ++i) {
        DFH_REQUIRE(std::isfinite(verts[i]), "%s: vertex %ld has a coordinate that is not finite", what, i / 3);
        maxabs = std::fmax(maxabs, std::fabs(verts[i]));
    }
    for (long i = 0; i < 3 * n_faces; ++i)
        DFH_REQUIRE(faces[i] >= 0 && faces[i] < n_verts, "%s: face %ld has vertex index %d outside [0, %ld)", what, i / 3, faces[i], n_verts);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, mean = 0.0;
    long kept = 0;
    for (long f = 0; f < n_faces; ++f) {
        if (!keep[f]) continue;
        ++kept;
        double ext = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double xa = verts[3 * (long)faces[3 * f] + a], xb = verts[3 * (long)faces[3 * f + 1] + a], xc = verts[3 * (long)faces[3 * f + 2] + a];
            const double mn = std::fmin(xa, std::fmin(xb, xc)), mx = std::fmax(xa, std::fmax(xb, xc));
            lo[a] = std::fmin(lo[a], mn); hi[a] = std::fmax(hi[a], mx);
            ext = std::fmax(ext, mx - mn);
        }
        mean += ext;
    }
    DFH_REQUIRE(kept > 0, "%s: every face has zero area", what);
    const double extent = std::fmax(hi[0] - lo[0], std::fmax(hi[1] - lo[1], hi[2] - lo[2]));
    DFH_REQUIRE(std::isfinite(extent) && std::isfinite(mean), "%s: the mesh's box overflows", what);
    // chosen cell: twice the mean face extent; never so small that an axis needs more than kMsdMaxDim cells
    double h = cell > 0.0 ? cell : 2.0 * (mean / (double)kept);
    h = std::fmax(h, extent / (double)(kMsdMaxDim - 1));
    DFH_REQUIRE(h > 0.0 && std::isfinite(h) && std::isfinite(1.0 / h), "%s: unusable cell size %g", what, h);
    const double inv_h = 1.0 / h;
    for (int a = 0; a < 3; ++a) {
        out->lo[a] = lo[a]; out->hi[a] = hi[a];
        const double n = std::floor((hi[a] - lo[a]) * inv_h) + 1.0;
        out->dims[a] = n < 1.0 ? 1 : n > (double)kMsdMaxDim ? kMsdMaxDim : (int)n;
    }
    long n_entries = 0;
    for (long f = 0; f < n_faces; ++f) {
        if (!keep[f]) continue;
        long cells = 1;
        for (int a = 0; a < 3; ++a) {
            const double xa = verts[3 * (long)faces[3 * f] + a], xb = verts[3 * (long)faces[3 * f + 1] + a], xc = verts[3 * (long)faces[3 * f + 2] + a];
            const int c0 = msd_cell(std::fmin(xa, std::fmin(xb, xc)), lo[a], h, inv_h, out->dims[a]);
            const int c1 = msd_cell(std::fmax(xa, std::fmax(xb, xc)), lo[a], h, inv_h, out->dims[a]);
            cells *= (c1 - c0 + 1);
        }
        n_entries += cells;
        DFH_REQUIRE(n_entries < (1l << 31), "%s: the cell table would hold 2^31 entries or more (cell %g too small for this mesh)", what, h);
    }
    out->cell = h;
    out->maxabs = maxabs;
    out->n_verts = n_verts;
    out->n_faces = n_faces;
    out->n_entries = n_entries;
    out->bytes = msd_table_bytes(out->dims, n_faces, n_entries);
    return DFH_OK;
}

extern "C" int dfh_mesh_sdf_build(const dfh_mesh_sdf *m, void *stream) {
    const char *what = "dfh_mesh_sdf_build";
    if (int rc = msd_check_mesh(what, m)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const MsdTable t = msd_table(m);
    const long nc = (long)t.n[0] * t.n[1] * t.n[2];
    DFH_HIP_CHECK(hipMemsetAsync(t.cursor, 0, (size_t)nc * 4, s));
    const unsigned blocks = (unsigned)((t.n_faces + 255) / 256);
    hipLaunchKernelGGL(msd_bin_kernel<false>, dim3(blocks), dim3(256), 0, s, t, m->verts, m->faces, m->keep);
    hipLaunchKernelGGL(msd_scan_kernel, dim3(1), dim3(1024), 0, s, t, nc);
    hipLaunchKernelGGL(msd_bin_kernel<true>, dim3(blocks), dim3(256), 0, s, t, m->verts, m->faces, m->keep);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

extern "C" int dfh_mesh_sdf_points(const dfh_mesh_sdf *m, const double *points, long n, double band, int orientation, double *sdist,
                                   float *closest, int *face, void *stream) {
    const char *what = "dfh_mesh_sdf_points";
    if (int rc = msd_check_mesh(what, m)) return rc;
    DFH_REQUIRE(n >= 0 && n < (1l << 31), "%s: bad point count %ld", what, n);
    DFH_REQUIRE(n == 0 || (points && sdist), "%s: null points or sdist", what);
    if (int rc = msd_check_band(what, band, orientation)) return rc;
    if (n == 0) return DFH_OK;
    MsdQuery q = {};
    msd_query_common(q, m, band, orientation);
    q.points = points; q.n_points = n;
    q.n_waves = (n + 63) / 64;
    q.value = sdist; q.status = nullptr; q.closest = closest; q.face = face;
    hipLaunchKernelGGL((msd_query_kernel<double, false>), dim3((unsigned)q.n_waves), dim3(64), 0, (hipStream_t)stream, q);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

template <typename VT>
static int msd_grid_launch(const MsdQuery &q, const dfh_mesh_sdf_grid_params *g, hipStream_t s) {
    hipLaunchKernelGGL((msd_query_kernel<VT, true>), dim3((unsigned)q.n_waves), dim3(64), 0, s, q);
    if (q.status) {
        const int X = q.X, Y = q.Y, Z = q.Z;
        VT *v = (VT *)g->value;
        hipLaunchKernelGGL((msd_fill_kernel<VT, 2>), dim3((unsigned)(((long)X * Y + 255) / 256)), dim3(256), 0, s, v, q.status, X, Y, Z, q.band);
        hipLaunchKernelGGL((msd_fill_kernel<VT, 1>), dim3((unsigned)(((long)X * Z + 255) / 256)), dim3(256), 0, s, v, q.status, X, Y, Z, q.band);
        hipLaunchKernelGGL((msd_fill_kernel<VT, 0>), dim3((unsigned)(((long)Y * Z + 255) / 256)), dim3(256), 0, s, v, q.status, X, Y, Z, q.band);
    }
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

extern "C" int dfh_mesh_sdf_grid(const dfh_mesh_sdf *m, const dfh_mesh_sdf_grid_params *g, void *stream) {
    const char *what = "dfh_mesh_sdf_grid";
    if (int rc = msd_check_mesh(what, m)) return rc;
    DFH_REQUIRE(g, "%s: null grid params", what);
    DFH_REQUIRE(g->value, "%s: null value", what);
    DFH_REQUIRE(g->dtype == DFH_F32 || g->dtype == DFH_F64, "%s: bad dtype %d", what, g->dtype);
    if (int rc = msd_check_band(what, g->band, g->orientation)) return rc;
    double max_sp = 0.0;
    for (int a = 0; a < 3; ++a) {
        DFH_REQUIRE(g->shape[a] >= 1, "%s: bad shape %dx%dx%d", what, g->shape[0], g->shape[1], g->shape[2]);
        DFH_REQUIRE(std::isfinite(g->origin[a]), "%s: origin is not finite", what);
        DFH_REQUIRE(g->spacing[a] > 0.0 && std::isfinite(g->spacing[a]), "%s: spacing must be finite and > 0, got %g", what, g->spacing[a]);
        max_sp = std::fmax(max_sp, g->spacing[a]);
    }
    DFH_REQUIRE((long)g->shape[0] * g->shape[1] * g->shape[2] < (1l << 31) && (long)g->shape[0] * g->shape[1] < (1l << 31)
                && (long)g->shape[1] * g->shape[2] < (1l << 31), "%s: grid of 2^31 vertices or more", what);
    const bool finite = std::isfinite(g->band);
    if (finite) {
        DFH_REQUIRE(g->band >= max_sp, "%s: the far fill needs band >= max(spacing): band %g, spacing %g", what, g->band, max_sp);
        DFH_REQUIRE(g->status, "%s: a finite band needs the status workspace", what);
    }
    MsdQuery q = {};
    msd_query_common(q, m, g->band, g->orientation);
    for (int a = 0; a < 3; ++a) { q.origin[a] = g->origin[a]; q.spacing[a] = g->spacing[a]; }
    q.X = g->shape[0]; q.Y = g->shape[1]; q.Z = g->shape[2];
    q.nbx = (q.X + 3) / 4; q.nby = (q.Y + 3) / 4; q.nbz = (q.Z + 3) / 4;
    q.n_waves = (long)q.nbx * q.nby * q.nbz;
    q.value = g->value; q.status = finite ? g->status : nullptr; q.closest = g->closest; q.face = g->face;
    return g->dtype == DFH_F32 ? msd_grid_launch<float>(q, g, (hipStream_t)stream) : msd_grid_launch<double>(q, g, (hipStream_t)stream);
}
