// K20  ray cast: depth, normal, colour and hit maps of a TSDF volume from up to 16 cameras (dfh_raycast), and the brick table
// that lets the march step over empty space (dfh_raycast_table).  No reference counterpart.  The semantics are written out
// operation by operation in include/dfusion_hip.h; tests/raycast_np.py restates them and agrees bit for bit.
//
// Shape.  One lane per pixel, a wave owns an 8 x 8-pixel tile (a workgroup 16 x 16), so that neighbouring rays walk through the
// same cells and table bytes and their gathers hit the same lines.  blockIdx.z is the view: the view's record is read from the
// kernel-argument segment through scalar loads at a wave-uniform offset.  A sample requests its eight corners as four z-adjacent
// pairs (load_pair of dfh_assoc_volume.h), all before the first use.  No LDS, no scratch, no private arrays, no atomics.  The
// kernel is instantiated per volume dtype, "w is read", "colour wanted" and "table given": none of these is a branch in the march.
//
// Why skipping gives the same bits.  The plain march evaluates sample k = 0, 1, .. kmax in turn; the only state it carries from
// one sample to the next is "the previous sample was known and > 0, at (za, ta)".  Write cell(k) for the clamped cell S() computes
// for sample k, brick(k) for the brick that cell belongs to.
//  (1) A dead brick's table entry says: every voxel in [8b - 1, 8b + 9]^3 (cut at the slab) holds T >= m > 0 with m > M 2^-30.
//      A trilinear value is three nested a + f (b - a) steps.  For f in [-2^-20, 1 + 2^-20] and a, b in [m, M] each step's exact
//      value is >= m - 2^-20 M, and its two roundings lose at most 2^-51 M more; so the computed t >= m - 2^-18 M > 0: a sample
//      all of whose corners lie in that voxel set is never <= 0, hence never a crossing (it may be unknown, which is no crossing
//      either).  Its only effect on the walk is the state it leaves for the NEXT sample.
//  (2) The march looks up brick(k) from the very cell S() would use.  If it is dead, the samples k' > k whose exact position lies in
//      the brick's closed box are found in closed form: the box's exit parameter zx along the ray and kn = floor((zx - zlo)/dz).
//      The computed i(z_k') differs from the exact line by far less than one voxel (the products and sums of step 1 carry 2^-52
//      relative error on values below 2^30 voxels for any camera within 2^30 voxels of the grid, the reciprocals used for zx
//      and kn 2^-51 more: below 2^-20 voxel in all), and sample k itself lies within that of the box.  So every skipped sample's
//      cell has all its corners in [8b - 1, 8b + 9]^3 and fractions in [-2^-20, 1 + 2^-20]: by (1) none of them is a crossing.
//      That is what the ring around the brick is for: the skip arithmetic needs to be right to a voxel, not to an ulp, and it is
//      not part of the restated semantics.
//  (3) After a skip the state is unknown ("stale").  When the march arrives at a sample k whose brick is live it first evaluates
//      sample k - 1 -- the same S(i(z_{k-1})) the plain march evaluated, z_{k-1} being a product, not a running sum -- which by (2)
//      is no crossing and leaves exactly the state the plain march has in front of sample k; then sample k.  If brick(k) is dead
//      again, sample k - 1 is never needed.  From there on both marches run the same operations on the same values.  A live
//      brick is looked up once: its samples up to the box's exit are evaluated without another lookup.  Evaluating a sample is
//      the plain march's own operation, so how many are evaluated before the next lookup cannot change a bit; only a SKIP needs
//      the proof.
// The root, the normal and the colour are computed after the walk from (za, ta, zb, tb) alone.
#include <cmath>

#include "dfh_assoc_volume.h"

namespace dfh {

constexpr int kRayMaxViews = 16;
constexpr int kRayBrick = 8;            // cells per brick side
constexpr int kRayTile = 16;            // pixels per workgroup side (four 8 x 8 wave tiles)

struct RayView { double wl[12]; };      // camera -> world, 3x4 row-major

// 1.8 KB by value in the kernel-argument segment
struct RayArgs {
    Mat3 Kinv;
    double scale, cx, cy, cz, half;
    double z_near, z_far, step, min_weight;
    int H, W;
    int X, Y, Z, x0, x1;
    int nb1, nb2;
    int refine, max_steps;
    RayView v[kRayMaxViews];
};

// the clamped cell of S(p): lo <= c <= hi - 1 whatever p is (a NaN gives lo)
__device__ __forceinline__ void ray_cell(const RayArgs &a, double p0, double p1, double p2, double &c0, double &c1, double &c2) {
    const double lo0 = (double)a.x0, m0 = (double)(a.x1 - 2), m1 = (double)(a.Y - 2), m2 = (double)(a.Z - 2);
    c0 = floor(p0); c1 = floor(p1); c2 = floor(p2);
    c0 = c0 >= lo0 ? c0 : lo0;  c0 = c0 <= m0 ? c0 : m0;
    c1 = c1 >= 0.0 ? c1 : 0.0;  c1 = c1 <= m1 ? c1 : m1;
    c2 = c2 >= 0.0 ? c2 : 0.0;  c2 = c2 <= m2 ? c2 : m2;
}

// S(p): returns known, t <- the trilinear value
template <typename VT, bool READ_W>
__device__ __forceinline__ bool ray_value(const VT *__restrict__ T, const VT *__restrict__ Wt, const RayArgs &a, double p0, double p1,
                                          double p2, double &t) {
    double c0, c1, c2;
    ray_cell(a, p0, p1, p2, c0, c1, c2);
    const double f0 = p0 - c0, f1 = p1 - c1, f2 = p2 - c2;
    const size_t sy = (size_t)a.Z, sx = (size_t)a.Y * sy;
    const size_t cell = (size_t)((int)c0 - a.x0) * sx + (size_t)(int)c1 * sy + (size_t)(int)c2;
    const VT *tc = T + cell;
    const LivePair<VT> r00 = load_pair(tc), r01 = load_pair(tc + sy), r10 = load_pair(tc + sx), r11 = load_pair(tc + sx + sy);
    bool known = true;
    if (READ_W) {
        const VT *wc = Wt + cell;
        const LivePair<VT> w00 = load_pair(wc), w01 = load_pair(wc + sy), w10 = load_pair(wc + sx), w11 = load_pair(wc + sx + sy);
        const double mw = a.min_weight;
        known = ((double)w00.lo >= mw) & ((double)w00.hi >= mw) & ((double)w01.lo >= mw) & ((double)w01.hi >= mw) &
                ((double)w10.lo >= mw) & ((double)w10.hi >= mw) & ((double)w11.lo >= mw) & ((double)w11.hi >= mw);
    }
    const double u000 = (double)r00.lo, u001 = (double)r00.hi, u010 = (double)r01.lo, u011 = (double)r01.hi;
    const double u100 = (double)r10.lo, u101 = (double)r10.hi, u110 = (double)r11.lo, u111 = (double)r11.hi;
    const double dz00 = u001 - u000, dz01 = u011 - u010, dz10 = u101 - u100, dz11 = u111 - u110;
    const double e00 = u000 + f2 * dz00, e01 = u010 + f2 * dz01, e10 = u100 + f2 * dz10, e11 = u110 + f2 * dz11;
    const double h0 = e00 + f1 * (e01 - e00), h1 = e10 + f1 * (e11 - e10);
    t = h0 + f0 * (h1 - h0);
    return known;
}

template <typename VT, bool READ_W, bool COLOR, bool TABLE>
__global__ __launch_bounds__(256) void raycast_kernel(const VT *__restrict__ T, const VT *__restrict__ Wt, const float4 *__restrict__ C,
                                                       const unsigned char *__restrict__ table, float *__restrict__ depth,
                                                       float *__restrict__ normals, unsigned *__restrict__ color,
                                                       float *__restrict__ hit, const RayArgs a) {
    const int view = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = (int)blockIdx.x * kRayTile + (wave & 1) * 8 + (lane & 7);
    const int y = (int)blockIdx.y * kRayTile + (wave >> 1) * 8 + (lane >> 3);
    if (x >= a.W || y >= a.H) return;
    const double *wl = a.v[view].wl;
    const size_t pix = ((size_t)view * a.H + y) * a.W + x;

    // 1. ray
    const double X = (double)x, Y = (double)y;
    const double rho0 = (a.Kinv.m[0] * X + a.Kinv.m[1] * Y) + a.Kinv.m[2];
    const double rho1 = (a.Kinv.m[3] * X + a.Kinv.m[4] * Y) + a.Kinv.m[5];
    const double rho2 = (a.Kinv.m[6] * X + a.Kinv.m[7] * Y) + a.Kinv.m[8];
    const double d0 = (wl[0] * rho0 + wl[1] * rho1) + wl[2] * rho2;
    const double d1 = (wl[4] * rho0 + wl[5] * rho1) + wl[6] * rho2;
    const double d2 = (wl[8] * rho0 + wl[9] * rho1) + wl[10] * rho2;
    const double o0 = (wl[3] - a.cx) / a.scale + a.half;
    const double o1 = (wl[7] - a.cy) / a.scale + a.half;
    const double o2 = (wl[11] - a.cz) / a.scale + a.half;
    const double e0 = d0 / a.scale, e1 = d1 / a.scale, e2 = d2 / a.scale;
    const double L = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    bool alive = (L > 0.0) & (L < __builtin_huge_val());

    // 2. clip
    const double lo0 = (double)a.x0, hi0 = (double)(a.x1 - 1), hi1 = (double)(a.Y - 1), hi2 = (double)(a.Z - 1);
    double zlo = a.z_near, zhi = a.z_far;
    {
        const double t1 = (lo0 - o0) / e0, t2 = (hi0 - o0) / e0;
        const double tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1;
        if (e0 == 0.0) alive = alive & (o0 >= lo0) & (o0 <= hi0);
        else { zlo = tn > zlo ? tn : zlo; zhi = tf < zhi ? tf : zhi; }
    }
    {
        const double t1 = (0.0 - o1) / e1, t2 = (hi1 - o1) / e1;
        const double tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1;
        if (e1 == 0.0) alive = alive & (o1 >= 0.0) & (o1 <= hi1);
        else { zlo = tn > zlo ? tn : zlo; zhi = tf < zhi ? tf : zhi; }
    }
    {
        const double t1 = (0.0 - o2) / e2, t2 = (hi2 - o2) / e2;
        const double tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1;
        if (e2 == 0.0) alive = alive & (o2 >= 0.0) & (o2 <= hi2);
        else { zlo = tn > zlo ? tn : zlo; zhi = tf < zhi ? tf : zhi; }
    }
    alive = alive & (zlo <= zhi);

    // 3./4. samples and walk
    const double dz = a.step / L;
    const double nd = floor((zhi - zlo) / dz);
    const int kmax = alive ? (nd < (double)a.max_steps ? (int)nd : a.max_steps) : -1;     // (a NaN nd: max_steps)
    double za = 0.0, ta = 0.0, zb = 0.0, tb = 0.0;
    bool have = false, crossed = false;
    // skip arithmetic (TABLE only; not part of the restated semantics: right to a voxel is enough, see the proof above)
    const double inv_dz = 1.0 / dz;
    const double r0 = 1.0 / e0, r1 = 1.0 / e1, r2 = 1.0 / e2;
    bool stale = false;
    int k = 0, kend = -1;
    // One flat loop: an iteration does at most one lookup and at most one evaluation, so that the lanes of a wave that step over
    // dead bricks and the lanes that sample advance together (a `continue` after the skip makes the compiler nest a skip loop
    // inside, in which every lane waits for the wave's longest run of dead bricks before it may sample: 5 x slower on the
    // bench scene).
    while (k <= kmax) {
        bool eval = true;
        if (TABLE && k > kend) {                                        // sample k is the first of a brick: one lookup per brick
            const double zk = zlo + (double)k * dz;
            double c0, c1, c2;
            ray_cell(a, o0 + zk * e0, o1 + zk * e1, o2 + zk * e2, c0, c1, c2);
            const int b0 = ((int)c0 - a.x0) >> 3, b1 = (int)c1 >> 3, b2 = (int)c2 >> 3;
            const bool live = table[((size_t)b0 * a.nb1 + b1) * a.nb2 + b2] != 0;
            const double inf = __builtin_huge_val();
            const double f0 = (double)(a.x0 + 8 * b0 + (e0 > 0.0 ? 8 : 0)), f1 = (double)(8 * b1 + (e1 > 0.0 ? 8 : 0)),
                         f2 = (double)(8 * b2 + (e2 > 0.0 ? 8 : 0));
            const double x0z = e0 == 0.0 ? inf : (f0 - o0) * r0, x1z = e1 == 0.0 ? inf : (f1 - o1) * r1,
                         x2z = e2 == 0.0 ? inf : (f2 - o2) * r2;
            double zx = x0z < x1z ? x0z : x1z;
            zx = x2z < zx ? x2z : zx;
            const double kd = floor((zx - zlo) * inv_dz);              // the last sample inside the box
            const int klast = kd < (double)kmax ? (kd > (double)k ? (int)kd : k) : kmax;
            eval = live;
            kend = klast;                                               // live: evaluated up to the box's end without another lookup
            if (!live) {                                                // dead: over the box without a sample
                k = klast + 1;
                stale = true;
                have = false;
            }
        }
        if (eval) {
            const int kk = (TABLE && stale) ? k - 1 : k;                 // (stale only after a skip: k >= 1)
            const double z = zlo + (double)kk * dz;
            double t;
            const bool known = ray_value<VT, READ_W>(T, Wt, a, o0 + z * e0, o1 + z * e1, o2 + z * e2, t);
            if (known & (t <= 0.0) & have) {
                zb = z; tb = t;
                crossed = true;
                k = kmax + 1;                                           // the walk ends
            } else {
                have = known & (t > 0.0);
                za = z; ta = t;
                k = kk + 1;
                stale = false;
            }
        }
    }

    // 5. root
    double zs = za + (zb - za) * (ta / (ta - tb));
    if (crossed) {
#pragma unroll 1
        for (int r = 0; r < a.refine; ++r) {
            double t;
            if (!ray_value<VT, READ_W>(T, Wt, a, o0 + zs * e0, o1 + zs * e1, o2 + zs * e2, t)) break;
            if (t > 0.0) { za = zs; ta = t; } else { zb = zs; tb = t; }
            zs = za + (zb - za) * (ta / (ta - tb));
        }
    }

    // 6. outputs
    const double p0 = o0 + zs * e0, p1 = o1 + zs * e1, p2 = o2 + zs * e2;
    if (depth) depth[pix] = crossed ? (float)(-zs) : 0.0f;
    if (hit) {
        const float qnan = __uint_as_float(0x7fc00000u);
        hit[3 * pix] = crossed ? (float)p0 : qnan;
        hit[3 * pix + 1] = crossed ? (float)p1 : qnan;
        hit[3 * pix + 2] = crossed ? (float)p2 : qnan;
    }
    if (normals) {
        double n0 = 0.0, n1 = 0.0, n2 = 0.0;
        if (crossed) {
            double g0 = 0.0, g1 = 0.0, g2 = 0.0;
            bool ok = true;
#pragma unroll 1
            for (int j = 0; j < 6; ++j) {
                const int ax = j >> 1;
                const double sgn = (j & 1) ? -1.0 : 1.0;
                const double q0 = ax == 0 ? p0 + sgn : p0, q1 = ax == 1 ? p1 + sgn : p1, q2 = ax == 2 ? p2 + sgn : p2;
                const bool inside = (q0 >= lo0) & (q0 <= hi0) & (q1 >= 0.0) & (q1 <= hi1) & (q2 >= 0.0) & (q2 <= hi2);
                double t;
                const bool known = ray_value<VT, READ_W>(T, Wt, a, q0, q1, q2, t);
                ok = ok & inside & known;
                const double st = sgn * t;
                g0 = ax == 0 ? g0 + st : g0;
                g1 = ax == 1 ? g1 + st : g1;
                g2 = ax == 2 ? g2 + st : g2;
            }
            const double sg = a.scale > 0.0 ? 1.0 : -1.0;
            const double m0 = sg * ((wl[0] * g0 + wl[4] * g1) + wl[8] * g2);
            const double m1 = sg * ((wl[1] * g0 + wl[5] * g1) + wl[9] * g2);
            const double m2 = sg * ((wl[2] * g0 + wl[6] * g1) + wl[10] * g2);
            const double l2 = (m0 * m0 + m1 * m1) + m2 * m2;
            if (ok & (l2 > 0.0) & (l2 < __builtin_huge_val())) {
                const double l = sqrt(l2);
                n0 = m0 / l; n1 = m1 / l; n2 = m2 / l;
                const double c = (n0 * (zs * rho0) + n1 * (zs * rho1)) + n2 * (zs * rho2);
                if (c > 0.0) { n0 = -n0; n1 = -n1; n2 = -n2; }
            }
        }
        normals[3 * pix] = (float)n0; normals[3 * pix + 1] = (float)n1; normals[3 * pix + 2] = (float)n2;
    }
    if (COLOR) {
        // sample_colors_kernel's rule (dfh_color.hip), statement for statement, at p
        unsigned rgbx = 0u;
        const bool in = crossed && (p0 >= 0.0) && (p0 <= (double)(a.X - 1)) && (p1 >= 0.0) && (p1 <= (double)(a.Y - 1)) && (p2 >= 0.0) &&
                        (p2 <= (double)(a.Z - 1));
        if (in) {
            const int ix = max(min((int)floor(p0), a.X - 2), 0), iy = max(min((int)floor(p1), a.Y - 2), 0),
                      iz = max(min((int)floor(p2), a.Z - 2), 0);
            const double fx = p0 - (double)ix, fy = p1 - (double)iy, fz = p2 - (double)iz;
            double S = 0.0, sr = 0.0, sg = 0.0, sb = 0.0;
#pragma unroll
            for (int corner = 0; corner < 8; ++corner) {
                const int dx = corner >> 2, dy = (corner >> 1) & 1, dzc = corner & 1;
                const int cx = ix + dx, cy = iy + dy, cz = iz + dzc;
                if (cx < a.x0 || cx >= a.x1 || cy >= a.Y || cz >= a.Z) continue;
                const float4 c = C[((size_t)(cx - a.x0) * a.Y + cy) * a.Z + cz];
                if (!(c.w > 0.f)) continue;
                const double wx = dx ? fx : 1.0 - fx, wy = dy ? fy : 1.0 - fy, wz = dzc ? fz : 1.0 - fz;
                const double tw = (wx * wy) * wz;
                S = S + tw;
                sr = sr + tw * (double)c.x;
                sg = sg + tw * (double)c.y;
                sb = sb + tw * (double)c.z;
            }
            if (S != 0.0) {
                const double qr = sr / S, qg = sg / S, qb = sb / S;
                const unsigned br = qr > 0.0 ? (qr >= 255.0 ? 255u : (unsigned)rint(qr)) : 0u;
                const unsigned bg = qg > 0.0 ? (qg >= 255.0 ? 255u : (unsigned)rint(qg)) : 0u;
                const unsigned bb = qb > 0.0 ? (qb >= 255.0 ? 255u : (unsigned)rint(qb)) : 0u;
                rgbx = br | (bg << 8) | (bb << 16) | (255u << 24);
            }
        }
        color[pix] = rgbx;
    }
}

// every pixel a miss (a slab without a cell)
__global__ __launch_bounds__(256) void raycast_miss_kernel(float *__restrict__ depth, float *__restrict__ normals,
                                                            unsigned *__restrict__ color, float *__restrict__ hit, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (depth) depth[i] = 0.0f;
    if (normals) { normals[3 * i] = 0.0f; normals[3 * i + 1] = 0.0f; normals[3 * i + 2] = 0.0f; }
    if (color) color[i] = 0u;
    if (hit) {
        const float qnan = __uint_as_float(0x7fc00000u);
        hit[3 * i] = qnan; hit[3 * i + 1] = qnan; hit[3 * i + 2] = qnan;
    }
}

// one wave per brick: the least and greatest T of voxels 8b - 1 .. 8b + 9 per axis (slab-local on axis 0), cut at the slab
template <typename VT>
__global__ __launch_bounds__(64) void raycast_table_kernel(const VT *__restrict__ T, unsigned char *__restrict__ table, int nx, int Y,
                                                           int Z, int nb1, int nb2) {
    const unsigned b = blockIdx.x;
    const int b2 = (int)(b % (unsigned)nb2), b1 = (int)((b / (unsigned)nb2) % (unsigned)nb1), b0 = (int)(b / ((unsigned)nb2 * (unsigned)nb1));
    constexpr int S = kRayBrick + 3;                  // 11 voxels per axis
    double mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    int bad = 0;
    for (int i = threadIdx.x; i < S * S * S; i += 64) {
        const int v2 = kRayBrick * b2 - 1 + i % S, v1 = kRayBrick * b1 - 1 + (i / S) % S, v0 = kRayBrick * b0 - 1 + i / (S * S);
        if (v0 < 0 || v0 >= nx || v1 < 0 || v1 >= Y || v2 < 0 || v2 >= Z) continue;
        const double t = (double)T[((size_t)v0 * Y + v1) * Z + v2];
        if (!(t > 0.0)) bad = 1;                       // <= 0 or NaN
        mn = t < mn ? t : mn;
        mx = t > mx ? t : mx;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double on = __shfl_xor(mn, s), ox = __shfl_xor(mx, s);
        mn = on < mn ? on : mn;
        mx = ox > mx ? ox : mx;
    }
    if (!(mn > mx * 0x1p-30)) bad = 1;
    const int live = __any(bad);
    if (threadIdx.x == 0) table[b] = live ? 1 : 0;
}

static bool ray_bricks(const dfh_slab &sl, long &nb0, long &nb1, long &nb2) {
    nb0 = (sl.x1 - sl.x0 + kRayBrick - 1) / kRayBrick;
    nb1 = (sl.res[1] + kRayBrick - 1) / kRayBrick;
    nb2 = (sl.res[2] + kRayBrick - 1) / kRayBrick;
    return nb0 * nb1 * nb2 < (1L << 31);
}

template <typename VT, bool READ_W, bool COLOR>
static void launch_raycast(const dfh_raycast_params &p, const RayArgs &a, bool use_table, hipStream_t s) {
    const dim3 grid((unsigned)((p.W + kRayTile - 1) / kRayTile), (unsigned)((p.H + kRayTile - 1) / kRayTile), (unsigned)p.n_views);
    const VT *T = static_cast<const VT *>(p.vol->tsdf), *Wt = static_cast<const VT *>(p.vol->tsdf_w);
    const float4 *C = COLOR ? reinterpret_cast<const float4 *>(p.colors->rgbw) : nullptr;
    unsigned *color = reinterpret_cast<unsigned *>(p.color);
    if (use_table)
        hipLaunchKernelGGL((raycast_kernel<VT, READ_W, COLOR, true>), grid, dim3(256), 0, s, T, Wt, C,
                           static_cast<const unsigned char *>(p.table), p.depth, p.normals, color, p.hit, a);
    else
        hipLaunchKernelGGL((raycast_kernel<VT, READ_W, COLOR, false>), grid, dim3(256), 0, s, T, Wt, C,
                           static_cast<const unsigned char *>(nullptr), p.depth, p.normals, color, p.hit, a);
}

template <typename VT>
static void launch_raycast_dtype(const dfh_raycast_params &p, const RayArgs &a, bool use_table, hipStream_t s) {
    const bool read_w = p.min_weight > 0.0, color = p.color != nullptr;
    if (read_w) { if (color) launch_raycast<VT, true, true>(p, a, use_table, s); else launch_raycast<VT, true, false>(p, a, use_table, s); }
    else { if (color) launch_raycast<VT, false, true>(p, a, use_table, s); else launch_raycast<VT, false, false>(p, a, use_table, s); }
}

}  // namespace dfh

extern "C" size_t dfh_raycast_table_bytes(const dfh_slab *slab) {
    using namespace dfh;
    if (check_slab("dfh_raycast_table_bytes", slab) != DFH_OK || slab->x0 == slab->x1) return 0;
    long nb0, nb1, nb2;
    if (!ray_bricks(*slab, nb0, nb1, nb2)) return 0;
    return (size_t)(nb0 * nb1 * nb2);
}

extern "C" int dfh_raycast_table(const dfh_volume *vol, void *table, void *stream) {
    using namespace dfh;
    static const char *const me = "dfh_raycast_table";
    const int rc = check_volume(me, vol);
    if (rc != DFH_OK) return rc;
    DFH_REQUIRE(table, "%s: null table", me);
    const dfh_slab &sl = vol->slab;
    if (sl.x0 == sl.x1) return DFH_OK;
    long nb0, nb1, nb2;
    DFH_REQUIRE(ray_bricks(sl, nb0, nb1, nb2), "%s: too many bricks", me);
    const dim3 grid((unsigned)(nb0 * nb1 * nb2));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vol->dtype == DFH_F64)
        hipLaunchKernelGGL(raycast_table_kernel<double>, grid, dim3(64), 0, s, static_cast<const double *>(vol->tsdf),
                           static_cast<unsigned char *>(table), sl.x1 - sl.x0, sl.res[1], sl.res[2], (int)nb1, (int)nb2);
    else
        hipLaunchKernelGGL(raycast_table_kernel<float>, grid, dim3(64), 0, s, static_cast<const float *>(vol->tsdf),
                           static_cast<unsigned char *>(table), sl.x1 - sl.x0, sl.res[1], sl.res[2], (int)nb1, (int)nb2);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

extern "C" int dfh_raycast(const dfh_raycast_params *p, void *stream) {
    using namespace dfh;
    static const char *const me = "dfh_raycast";
    DFH_REQUIRE(p, "%s: null params", me);
    const int rc = check_volume(me, p->vol);
    if (rc != DFH_OK) return rc;
    const dfh_slab &sl = p->vol->slab;
    DFH_REQUIRE(p->n_views >= 1 && p->n_views <= kRayMaxViews, "%s: %d views (1..%d per call)", me, p->n_views, kRayMaxViews);
    DFH_REQUIRE(p->lw && p->wl, "%s: null lw or wl", me);
    DFH_REQUIRE(p->H >= 1 && p->W >= 1 && (long)p->H * p->W < (1L << 31), "%s: bad image size %dx%d", me, p->H, p->W);
    DFH_REQUIRE(std::isfinite(p->step) && p->step > 0.0, "%s: step must be finite and > 0", me);
    DFH_REQUIRE(std::isfinite(p->z_near) && p->z_near >= 0.0, "%s: z_near must be finite and >= 0", me);
    DFH_REQUIRE(p->z_far > p->z_near, "%s: z_far must be > z_near", me);                       // (NaN fails, +inf passes)
    DFH_REQUIRE(p->min_weight >= 0.0, "%s: min_weight must be >= 0", me);                     // (NaN fails)
    DFH_REQUIRE(p->refine >= 0 && p->refine <= 8, "%s: refine=%d outside [0,8]", me, p->refine);
    DFH_REQUIRE(p->max_steps >= 1, "%s: max_steps must be >= 1", me);
    DFH_REQUIRE(std::isfinite(p->scale) && p->scale != 0.0, "%s: scale must be finite and non-zero", me);
    DFH_REQUIRE(p->depth || p->normals || p->color || p->hit, "%s: no output", me);
    if (p->color) {
        DFH_REQUIRE(p->colors && p->colors->rgbw, "%s: color wanted without a colour volume", me);
        const dfh_slab &cs = p->colors->slab;
        DFH_REQUIRE(cs.res[0] == sl.res[0] && cs.res[1] == sl.res[1] && cs.res[2] == sl.res[2] && cs.x0 == sl.x0 && cs.x1 == sl.x1,
                    "%s: the colour volume's slab is not the volume's", me);
    }
    const bool use_table = p->table != nullptr && opt().raycast_skip != 0;
    if (p->table)
        DFH_REQUIRE(p->table_bytes >= dfh_raycast_table_bytes(&sl), "%s: table too small (need %zu bytes)", me,
                    dfh_raycast_table_bytes(&sl));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t npix = (size_t)p->n_views * p->H * p->W;
    if (sl.x1 - sl.x0 < 2 || sl.res[1] < 2 || sl.res[2] < 2) {                                // no cell: every pixel a miss
        DFH_REQUIRE((npix + 255) / 256 < (1UL << 31), "%s: too many pixels", me);
        hipLaunchKernelGGL(raycast_miss_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, p->depth, p->normals,
                           reinterpret_cast<unsigned *>(p->color), p->hit, npix);
        DFH_HIP_CHECK(hipGetLastError());
        return DFH_OK;
    }
    DFH_REQUIRE((p->H + kRayTile - 1) / kRayTile <= 65535, "%s: image too tall", me);
    long nb0, nb1, nb2;
    DFH_REQUIRE(ray_bricks(sl, nb0, nb1, nb2), "%s: too many bricks", me);
    RayArgs a = {};
    for (int i = 0; i < 9; ++i) a.Kinv.m[i] = p->Kinv[i];
    a.scale = p->scale; a.cx = p->center[0]; a.cy = p->center[1]; a.cz = p->center[2]; a.half = p->half;
    a.z_near = p->z_near; a.z_far = p->z_far; a.step = p->step; a.min_weight = p->min_weight;
    a.H = p->H; a.W = p->W;
    a.X = sl.res[0]; a.Y = sl.res[1]; a.Z = sl.res[2]; a.x0 = sl.x0; a.x1 = sl.x1;
    a.nb1 = (int)nb1; a.nb2 = (int)nb2;
    a.refine = p->refine; a.max_steps = p->max_steps < (1 << 30) ? p->max_steps : (1 << 30);
    for (int v = 0; v < p->n_views; ++v)
        for (int i = 0; i < 12; ++i) a.v[v].wl[i] = p->wl[12 * v + i];
    if (p->vol->dtype == DFH_F64) launch_raycast_dtype<double>(*p, a, use_table, s);
    else launch_raycast_dtype<float>(*p, a, use_table, s);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}
