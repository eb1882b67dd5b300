// "Associate one sample and differentiate it": the device side that the data-row kernel of the normal-equation build
// (dfh_solve.hip) and the rigid-mode rows kernel (dfh_gn_global.hip) both run -- the projective association with
// fuseDepths' projection primitives (reference core/fusion_dm.py:191-200) and the analytic 6-DoF left-twist Jacobian row
// (derivation in oracle/gn_np.py, pinned against finite differences of the reference's residual) -- and the argument
// checks every GN entry point shares.
#pragma once
#include "dfh_solve_math.h"

namespace dfh {

// ------------------------------------------------------------------------------- association
struct AssocParams {
    Mat3 K, Kinv;
    DQ lw;
    double scale, inv_scale, cx, cy, cz, half, max_dist;
    int H, W, k;
};

// (blend_static, the normalised blend of a sample's k node DQs with its static weights: dfh_dq.h)
static_assert(kBlendKMax == kKMaxS, "blend_static reads kKMaxS index / weight slots");

// One live view of a frame in device memory (dfh_gn_pack_views): extrinsic, the inverse of its 3x3 part, the depth map.
struct AssocView {
    double lw_cam[12];
    double Rinv[9];
    const void *depth;
    const float *cells;      // per 16 x 16-pixel cell {smallest, largest valid z = -depth} (float32 maps); null: none
    double cull_ok;          // 1: this view's extrinsic is a rigid motion (the depth-interval test below is exact for it)
};                           // 192 bytes
static_assert(sizeof(AssocView) == 192, "AssocView is a 192-byte record");
constexpr int kCellPx = 16;

// Projective association of one warped sample xp (index space) against ONE view: project with the reference's primitives,
// take the nearest depth pixel, back-project -- in two halves: up to the pixel (no memory access), and from the pixel's depth
// on (validity before the distance gate; c = correspondence in index space, d2 = its squared distance from xp).
// associate_views runs the first half for several views, asks for their depth values together and only then goes on: one
// memory round trip per group of views instead of one per view.
__device__ __forceinline__ bool associate_project(const AssocParams &p, const double *lw, const D3 &xp, double &u, double &v) {
    // index -> world -> camera -> pixel (fusion_dm.py:191-195)
    const double wx = p.scale * (xp.x - p.half) + p.cx, wy = p.scale * (xp.y - p.half) + p.cy, wz = p.scale * (xp.z - p.half) + p.cz;
    const double l0 = ((lw[0] * wx + lw[1] * wy) + lw[2] * wz) + lw[3];
    const double l1 = ((lw[4] * wx + lw[5] * wy) + lw[6] * wz) + lw[7];
    const double l2 = ((lw[8] * wx + lw[9] * wy) + lw[10] * wz) + lw[11];
    const double p0 = (p.K.m[0] * l0 + p.K.m[1] * l1) + p.K.m[2] * l2;
    const double p1 = (p.K.m[3] * l0 + p.K.m[4] * l1) + p.K.m[5] * l2;
    const double p2 = (p.K.m[6] * l0 + p.K.m[7] * l1) + p.K.m[8] * l2;
    bool ok = p2 != 0.0;
    // one corrected reciprocal instead of two IEEE divisions (u, v within 1.5 ulp: the association has no reference counterpart
    // whose rounding would have to be met; the oracle comparison is to 1e-9)
    double rp = __builtin_amdgcn_rcp(p2);
    rp = __builtin_fma(rp, __builtin_fma(-p2, rp, 1.0), rp);
    rp = __builtin_fma(rp, __builtin_fma(-p2, rp, 1.0), rp);
    u = p0 * rp; v = p1 * rp;
    return ok && (u >= 0.0) && (u < (double)(p.W - 1)) && (v >= 0.0) && (v < (double)(p.H - 1));
}

// z = -depth[rint(v)][rint(u)] (:196) -> validity, correspondence c in index space, its squared distance d2 from xp
__device__ __forceinline__ bool associate_backproject(const AssocParams &p, const double *lw, const double *Rinv, double z, double u, double v,
                                                      const D3 &xp, double &c0, double &c1, double &c2, double &d2) {
    // back-projection K^-1 (z [u,v,1]) (:198-200), camera -> world -> index
    const double a0 = z * u, a1 = z * v, a2 = z * 1.0;
    const double q0 = (p.Kinv.m[0] * a0 + p.Kinv.m[1] * a1) + p.Kinv.m[2] * a2 - lw[3];
    const double q1 = (p.Kinv.m[3] * a0 + p.Kinv.m[4] * a1) + p.Kinv.m[5] * a2 - lw[7];
    const double q2 = (p.Kinv.m[6] * a0 + p.Kinv.m[7] * a1) + p.Kinv.m[8] * a2 - lw[11];
    const double X = (Rinv[0] * q0 + Rinv[1] * q1) + Rinv[2] * q2;
    const double Y = (Rinv[3] * q0 + Rinv[4] * q1) + Rinv[5] * q2;
    const double Z = (Rinv[6] * q0 + Rinv[7] * q1) + Rinv[8] * q2;
    c0 = (X - p.cx) * p.inv_scale + p.half;
    c1 = (Y - p.cy) * p.inv_scale + p.half;
    c2 = (Z - p.cz) * p.inv_scale + p.half;
    const double dx = c0 - xp.x, dy = c1 - xp.y, dz = c2 - xp.z;
    d2 = dx * dx + dy * dy + dz * dz;
    return z > 0.0;
}

// Several views (BASELINE config 5: the live frame is eight depth maps): every view is tried in turn, the sample keeps the
// correspondence of the view in which it lies CLOSEST to the observed surface (smallest |c - x'|; the gate is applied per
// view; ties go to the lower view index) -- one data row per sample, as with one view, so the block pattern and the plan do
// not depend on the number of views.  The reference has no counterpart: its correspondences are mesh-to-mesh
// (core/fusion.py:255-276); restated in oracle/gn_np.py:associate_depth_views.
// view_mask (wave-uniform): the views to try, bit v = view v (all of them: ~0u).  A tile of the fused build passes the views
// its samples can possibly be valid in (tile_view_mask below): the others are not even projected.
//
// The normal-compatibility gate (dfh_gn_normal_gate; GATED only -- the ungated instantiations read none of it): a view's
// correspondence also needs the live normal l of the pixel the depth came from (normals: n_views x H x W x 3 float32, camera
// space, (0,0,0) = none) to agree with the sample's warped normal n' = (npx, npy, npz) rotated into that camera, m = R n':
// d = sgn(scale) (m . l) > 0 and d^2 >= min_cos^2 |m|^2 |l|^2 (no square root; a NaN fails both ways round).  The three floats
// are asked for together with the depth value -- still one memory round trip per group of views -- and the test sits beside
// the distance gate, in front of the "nearest view wins" comparison: a rejected nearer view lets a farther compatible one win.
// It only removes correspondences, so tile_view_mask stays exact.  Restated in tests/assoc_normals_np.py.
struct NormalGate {
    const float *normals;
    double min_cos;
};

template <typename DepthT, bool GATED = false>
__device__ __forceinline__ bool associate_views(const AssocParams &p, const AssocView *__restrict__ views, int n_views, const D3 &xp,
                                                double (&c)[3], unsigned view_mask = ~0u, const float *__restrict__ normals = nullptr,
                                                double min_cos = 0.0, double npx = 0.0, double npy = 0.0, double npz = 0.0) {
    bool any = false;
    double best = __builtin_huge_val();
    c[0] = 0.0; c[1] = 0.0; c[2] = 0.0;
    constexpr int G = 4;                                   // views per group: their depth gathers are in flight together
    unsigned todo = view_mask & (n_views >= 32 ? ~0u : ((1u << n_views) - 1u));
    while (todo) {                                         // (uniform: the views' parameters come through scalar loads)
        double u[G], vv[G], z[G];
        float l[GATED ? G : 1][3];
        bool ok[G];
        int vi_[G];
#pragma unroll
        for (int j = 0; j < G; ++j) {
            ok[j] = false; z[j] = 0.0; u[j] = 0.0; vv[j] = 0.0;
            vi_[j] = -1;
            if constexpr (GATED) { l[j][0] = 0.0f; l[j][1] = 0.0f; l[j][2] = 0.0f; }
            if (todo) {
                const int v = __builtin_ctz(todo);         // (ascending: the surviving views in view order)
                todo &= todo - 1u;
                vi_[j] = v;
                ok[j] = associate_project(p, views[v].lw_cam, xp, u[j], vv[j]);
                if (ok[j]) {
                    const int ui = (int)rint(u[j]), vi = (int)rint(vv[j]);
                    z[j] = -1.0 * (double)static_cast<const DepthT *>(views[v].depth)[(size_t)vi * p.W + ui];     // :196
                    if constexpr (GATED) {
                        const float *ln = normals + (((size_t)v * p.H + vi) * p.W + ui) * 3;
                        l[j][0] = ln[0]; l[j][1] = ln[1]; l[j][2] = ln[2];
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < G; ++j) {                      // (in view order: ties go to the lower index)
            if (ok[j]) {
                double c0, c1, c2, d2;
                bool good = associate_backproject(p, views[vi_[j]].lw_cam, views[vi_[j]].Rinv, z[j], u[j], vv[j], xp, c0, c1, c2, d2);
                if (good && p.max_dist > 0.0) good = d2 <= p.max_dist * p.max_dist;
                if constexpr (GATED) {
                    const double *R = views[vi_[j]].lw_cam;
                    const double m0 = (R[0] * npx + R[1] * npy) + R[2] * npz;
                    const double m1 = (R[4] * npx + R[5] * npy) + R[6] * npz;
                    const double m2 = (R[8] * npx + R[9] * npy) + R[10] * npz;
                    const double l0 = (double)l[j][0], l1 = (double)l[j][1], l2 = (double)l[j][2];
                    const double sgn = p.scale > 0.0 ? 1.0 : -1.0;
                    const double d = sgn * ((m0 * l0 + m1 * l1) + m2 * l2);
                    const double mm = (m0 * m0 + m1 * m1) + m2 * m2, ll = (l0 * l0 + l1 * l1) + l2 * l2;
                    good = good && d > 0.0 && d * d >= (min_cos * min_cos) * (mm * ll);      // (a NaN fails)
                }
                // (strict, best starts at +inf: a depth of -inf -- c and d2 inf or NaN -- or a d2 that overflows is no data row, with
                // or without the gate; oracle/gn_np.py:associate_depth states the same rule)
                if (good && d2 < best) { best = d2; c[0] = c0; c[1] = c1; c[2] = c2; any = true; }
            }
        }
    }
    return any;
}

// Which views can hold a valid correspondence for ANY sample of a tile (round 4; exact: a dropped view yields none).
// A tile's samples share a node tuple, so their warped positions fill a small box B.  For a view with a rigid extrinsic and a
// pinhole K (K^-1's last row = (0, 0, 1)): a correspondence c is the back-projection of a pixel at camera depth z, the sample
// x' has camera depth l2(x'), and |c - x'| (index units) = |c_cam - l| / scale >= |z - l2| / scale.  With B in front of the
// camera its image lies inside the bounding rectangle of its eight projected corners and l2 over B inside the corners' range
// [l2min, l2max] (affine).  The view is dropped when the rectangle misses [0, W-1) x [0, H-1), or the pixels it can round to
// hold no valid depth, or their valid depths [zmin, zmax] (a table of 16 x 16-pixel cells, dfh_gn_pack_views) stay
// further than max_dist from [l2min, l2max].  Thread t of the tile takes corner t & 7 of view t >> 3 (n_views <= 16).
// All kTile threads call this; box = {xmin, xmax, ymin, ymax, zmin, zmax} of the tile's warped samples (an empty tile: min > max).
__device__ __forceinline__ unsigned tile_view_mask(const AssocParams &p, const AssocView *__restrict__ views, int n_views, const double (&box)[6],
                                                   unsigned *s_mask) {
    const int t = threadIdx.x;
    if (t == 0) *s_mask = 0u;
    __syncthreads();
    const int v = t >> 3, corner = t & 7;
    if (v < n_views) {                                                         // (whole groups of eight lanes)
        const AssocView &vw = views[v];
        const double *lw = vw.lw_cam;
        const D3 xp{(corner & 1) ? box[1] : box[0], (corner & 2) ? box[3] : box[2], (corner & 4) ? box[5] : box[4]};
        const double wx = p.scale * (xp.x - p.half) + p.cx, wy = p.scale * (xp.y - p.half) + p.cy, wz = p.scale * (xp.z - p.half) + p.cz;
        const double l0 = ((lw[0] * wx + lw[1] * wy) + lw[2] * wz) + lw[3];
        const double l1 = ((lw[4] * wx + lw[5] * wy) + lw[6] * wz) + lw[7];
        const double l2 = ((lw[8] * wx + lw[9] * wy) + lw[10] * wz) + lw[11];
        const double p0 = (p.K.m[0] * l0 + p.K.m[1] * l1) + p.K.m[2] * l2;
        const double p1 = (p.K.m[3] * l0 + p.K.m[4] * l1) + p.K.m[5] * l2;
        const double p2 = (p.K.m[6] * l0 + p.K.m[7] * l1) + p.K.m[8] * l2;
        bool front = p2 > 1e-9 && l2 > 1e-9;
        const double u = front ? p0 / p2 : 0.0, vv = front ? p1 / p2 : 0.0;
        double umin = u, umax = u, vmin = vv, vmax = vv, lmin = l2, lmax = l2;
#pragma unroll
        for (int o = 1; o <= 4; o <<= 1) {
            umin = fmin(umin, __shfl_xor(umin, o, 8)); umax = fmax(umax, __shfl_xor(umax, o, 8));
            vmin = fmin(vmin, __shfl_xor(vmin, o, 8)); vmax = fmax(vmax, __shfl_xor(vmax, o, 8));
            lmin = fmin(lmin, __shfl_xor(lmin, o, 8)); lmax = fmax(lmax, __shfl_xor(lmax, o, 8));
            front = front & (__shfl_xor(front ? 1 : 0, o, 8) != 0);
        }
        bool keep = true;
        const bool can = front && vw.cells != nullptr && vw.cull_ok == 1.0 && box[0] <= box[1] && p.max_dist > 0.0 &&
                         p.Kinv.m[6] == 0.0 && p.Kinv.m[7] == 0.0 && p.Kinv.m[8] == 1.0;
        if (can) {
            const double eps = 1e-6;                                           // pixels: the corners' own rounding is ~1e-12
            // samples are valid only for 0 <= u < W - 1, 0 <= v < H - 1 (associate_project)
            const double ua = fmax(umin - eps, 0.0), ub = fmin(umax + eps, (double)(p.W - 1));
            const double va = fmax(vmin - eps, 0.0), vb = fmin(vmax + eps, (double)(p.H - 1));
            if (ua > ub || va > vb) {
                keep = false;                                                  // the whole box projects outside the image
            } else {
                // pixels the samples can round to: [floor(ua), ceil(ub)] x [floor(va), ceil(vb)], inside the image
                const int x0 = (int)floor(ua), x1 = min((int)ceil(ub), p.W - 1), y0 = (int)floor(va), y1 = min((int)ceil(vb), p.H - 1);
                const int cx0 = x0 / kCellPx, cx1 = x1 / kCellPx, cy0 = y0 / kCellPx, cy1 = y1 / kCellPx;
                const int nx = cx1 - cx0 + 1, ncell = nx * (cy1 - cy0 + 1), ncx = (p.W + kCellPx - 1) / kCellPx;
                if (ncell <= 64) {                                             // (a larger footprint: keep the view)
                    float zlo = __builtin_huge_valf(), zhi = 0.0f;
                    for (int i = corner; i < ncell; i += 8) {
                        const int cy = cy0 + i / nx, cx = cx0 + i % nx;
                        const float2 mm = *reinterpret_cast<const float2 *>(vw.cells + 2 * ((size_t)cy * ncx + cx));
                        zlo = fminf(zlo, mm.x); zhi = fmaxf(zhi, mm.y);
                    }
#pragma unroll
                    for (int o = 1; o <= 4; o <<= 1) { zlo = fminf(zlo, __shfl_xor(zlo, o, 8)); zhi = fmaxf(zhi, __shfl_xor(zhi, o, 8)); }
                    const double md = p.max_dist * fabs(p.scale) * (1.0 + 1e-6) + 1e-9 * (1.0 + lmax);
                    if (!(zhi > 0.0f) || zlo > zhi) keep = false;              // no valid pixel under the box
                    else if (lmin - (double)zhi > md || (double)zlo - lmax > md) keep = false;
                }
            }
        }
        if (corner == 0 && keep) atomicOr(s_mask, 1u << v);
    }
    __syncthreads();
    return *s_mask;
}

struct BuildParams {
    DQ lw;
    int S, k, N;
    double huber;             // > 0: IRLS weight min(1, huber / |r|) on the data rows (the reference's solver runs
};                            //      least_squares(loss='huber'), f_scale 1: core/fusion.py:389); 0: plain least squares

constexpr int kTile = kGnTile;                  // samples (= threads) per tile, dfh_common.h
constexpr int kTileWaves = kTile / 64;

// scratch row of the planned build: {Gram matrix of the row's 6K Jacobian columns as 6x6 sub-blocks (slot sa <= slot sb), each
// stored WHOLE and row-major (36 contiguous doubles; the diagonal ones with both triangles) | J^T r | cost | count | live flag},
// padded to whole 64-byte lines.  The gather reads one sub-block per list entry: 288 contiguous bytes instead of 36 values strewn
// over a packed 24 x 24 triangle (6-12 cache lines) -- its traffic was 9x the live rows' size.
__host__ __device__ constexpr int gn_nsub(int K) { return K * (K + 1) / 2; }
__host__ __device__ constexpr int gn_sub(int K, int sa, int sb) { return sa * K - (sa * (sa - 1)) / 2 + (sb - sa); }   // sa <= sb
__host__ __device__ constexpr int gn_row_gram(int K) { return 36 * gn_nsub(K); }
__host__ __device__ constexpr int gn_row_entries(int K) { return gn_row_gram(K) + 6 * K + 2; }
__host__ __device__ constexpr int gn_row_stride(int K) { return (gn_row_entries(K) + 1 + 7) / 8 * 8; }
// element (ia, ib) of the Gram sub-block for tuple slots (sa, sb), any order, inside a scratch row
__host__ __device__ constexpr int gn_gram_index(int K, int sa, int sb, int ia, int ib) {
    return sa <= sb ? 36 * gn_sub(K, sa, sb) + 6 * ia + ib : 36 * gn_sub(K, sb, sa) + 6 * ib + ia;
}

// A sample's warped normal n' as data_row_from computes it for the row (the same functions on the same values: the same bits) --
// what the normal gate compares with the live normals, before the association.
__device__ __forceinline__ D3 warped_normal(const double *bh, const double *lwq, double nx, double ny, double nz) {
    const D3 n1 = dqb_warp_normal_exact(bh, round_f32(nx), round_f32(ny), round_f32(nz));
    return dqb_warp_normal_exact(lwq, round_f32(n1.x), round_f32(n1.y), round_f32(n1.z));
}

// Residual and 6-DoF Jacobian rows of one data sample (formulas: oracle/gn_np.py
// data_residual_jacobian).  J is written as k x 6 into Jrow (row-major), returns r.
// second half of data_row: from the normalised blend bh (|b|_8 = nb), the float32-rounded point pf and the warped point xp
__device__ __forceinline__ double data_row_from(const double *__restrict__ node_dq, const int *idx, const double *w, int k,
                                                const double *lwq, const double *bh, double nb, double pfx, double pfy, double pfz,
                                                const D3 &xp, double nx, double ny, double nz, double c0, double c1, double c2,
                                                double *Jrow);

__device__ __forceinline__ double data_row(const double *__restrict__ node_dq, const int *idx, const double *w, int k,
                                           const double *lwq, double px, double py, double pz, double nx, double ny,
                                           double nz, double c0, double c1, double c2, double *Jrow) {
    double bh[8];
    const double nb = blend_static(node_dq, idx, w, k, bh);
    const double pfx = round_f32(px), pfy = round_f32(py), pfz = round_f32(pz);
    const D3 x1 = dqb_warp_exact(bh, pfx, pfy, pfz);
    const D3 xp = dqb_warp_exact(lwq, round_f32(x1.x), round_f32(x1.y), round_f32(x1.z));
    return data_row_from(node_dq, idx, w, k, lwq, bh, nb, pfx, pfy, pfz, xp, nx, ny, nz, c0, c1, c2, Jrow);
}

__device__ __forceinline__ double data_row_from(const double *__restrict__ node_dq, const int *idx, const double *w, int k,
                                                const double *lwq, const double *bh, double nb, double pfx, double pfy, double pfz,
                                                const D3 &xp, double nx, double ny, double nz, double c0, double c1, double c2,
                                                double *Jrow) {
    const double nfx = round_f32(nx), nfy = round_f32(ny), nfz = round_f32(nz);
    const D3 n1 = dqb_warp_normal_exact(bh, nfx, nfy, nfz);
    const D3 np_ = dqb_warp_normal_exact(lwq, round_f32(n1.x), round_f32(n1.y), round_f32(n1.z));
    const double d0 = xp.x - c0, d1 = xp.y - c1, d2 = xp.z - c2;
    const double r = (np_.x * d0 + np_.y * d1) + np_.z * d2;
    // u = A^T n', h = A^T (x' - c),  A^T y = vec(rl* Y rl)
    const Q4 rl{lwq[0], lwq[1], lwq[2], lwq[3]};
    const Q4 rlc = qconj(rl);
    const Q4 U = qmul(qmul(rlc, qpure(np_.x, np_.y, np_.z)), rl);
    const Q4 Hq = qmul(qmul(rlc, qpure(d0, d1, d2)), rl);
    const Q4 Up = qpure(U.x, U.y, U.z), Hp = qpure(Hq.x, Hq.y, Hq.z);
    const Q4 rr{bh[0], bh[1], bh[2], bh[3]}, dd{bh[4], bh[5], bh[6], bh[7]};
    const Q4 Ur = qmul(Up, rr);
    Q4 g_r = qadd(qadd(qmul(Ur, qpure(pfx, pfy, pfz)), qmul(Up, dd)), qmul(qmul(Hp, rr), qpure(nfx, nfy, nfz)));
    g_r = qscale(g_r, -2.0);
    Q4 g_d = qscale(Ur, 2.0);
    const double gb = (g_r.w * bh[0] + g_r.x * bh[1] + g_r.y * bh[2] + g_r.z * bh[3]) +
                      (g_d.w * bh[4] + g_d.x * bh[5] + g_d.y * bh[6] + g_d.z * bh[7]);
    const double inv = 1.0 / nb;
    g_r = Q4{(g_r.w - gb * bh[0]) * inv, (g_r.x - gb * bh[1]) * inv, (g_r.y - gb * bh[2]) * inv, (g_r.z - gb * bh[3]) * inv};
    g_d = Q4{(g_d.w - gb * bh[4]) * inv, (g_d.x - gb * bh[5]) * inv, (g_d.y - gb * bh[6]) * inv, (g_d.z - gb * bh[7]) * inv};
#pragma unroll
    for (int j = 0; j < kKMaxS; ++j) {
        if (j < k) {
            const double *q = node_dq + 8 * idx[j];
            const Q4 rac{q[0], -q[1], -q[2], -q[3]}, dac{q[4], -q[5], -q[6], -q[7]};
            const Q4 a = qadd(qmul(g_r, rac), qmul(g_d, dac));
            const Q4 t = qmul(g_d, rac);
            const double hw = 0.5 * w[j];
            Jrow[6 * j + 0] = hw * a.x; Jrow[6 * j + 1] = hw * a.y; Jrow[6 * j + 2] = hw * a.z;
            Jrow[6 * j + 3] = hw * t.x; Jrow[6 * j + 4] = hw * t.y; Jrow[6 * j + 5] = hw * t.z;
        }
    }
    return r;
}

// What a kernel that associates is given (assoc_args below fills it from the problem and the frame).
struct AssocArgs {
    AssocParams ap;
    const AssocView *views;     // n_views views from a dfh_gn_pack_views table, of the kernel's depth type
    int n_views;
    int cull;                   // 1: drop, per tile, the views none of its samples can be valid in (tile_view_mask)
};
// ... and a kernel that associates through the normal gate (its own struct: the ungated kernels' arguments stay what they are)
struct GatedAssocArgs : AssocArgs {
    NormalGate ng;
};

// ------------------------------------------------------------------------------- host side
// What every GN entry point checks of its problem: the samples and nodes; with `system` also the block system and the plans.
inline int check_problem(const char *what, const dfh_gn_problem *p, bool system) {
    DFH_REQUIRE(p, "%s: null problem", what);
    DFH_REQUIRE(p->n_samples >= 0 && p->n_nodes >= 1, "%s: bad sizes", what);
    DFH_REQUIRE(p->knn >= 1 && p->knn <= kKMaxS, "%s: knn=%d outside [1,%d]", what, p->knn, kKMaxS);
    DFH_REQUIRE(p->huber_delta >= 0.0, "%s: negative huber_delta", what);
    DFH_REQUIRE(p->node_dq, "%s: null node_dq", what);
    if (p->n_samples > 0)
        DFH_REQUIRE(p->sample_pos && p->sample_nrm && p->nbr && p->weights && p->corr && p->valid, "%s: null sample pointer", what);
    if (!system) return DFH_OK;
    DFH_REQUIRE(p->n_blocks >= 1, "%s: bad sizes", what);
    DFH_REQUIRE(p->node_pos && p->node_w && p->row_ptr && p->col && p->vals && p->rhs && p->cost_count, "%s: null pointer", what);
    DFH_REQUIRE(p->n_upper >= 0 && p->n_upper <= p->n_blocks && (p->n_upper == 0 || p->blk_upper), "%s: bad upper-block list", what);
    if (p->blk_ptr) {
        // (a rank whose slab holds no surface has no samples, no rows and EMPTY entry lists: null pointers are fine then)
        DFH_REQUIRE(p->n_rows >= 0 && p->node_ptr && (p->n_rows == 0 || (p->blk_ent && p->node_ent)), "%s: null plan array", what);
        DFH_REQUIRE(p->n_samples == 0 || (p->run_id && p->partial && p->n_rows > 0), "%s: samples without rows", what);
        if (p->partial_reg)
            DFH_REQUIRE(p->rblk_ptr && p->rblk_ent && p->rnode_ptr && p->rnode_ent, "%s: null regulariser plan array", what);
    }
    return DFH_OK;
}

// ... and of its frame; `fused`: the association runs inside the data-row kernel, which reads float32 maps only.
inline int check_frame(const char *what, const dfh_gn_frame *f, bool fused) {
    DFH_REQUIRE(f, "%s: null frame", what);
    DFH_REQUIRE(f->views && f->n_views >= 1 && f->n_views <= DFH_GN_MAX_VIEWS, "%s: needs 1..%d packed views", what, DFH_GN_MAX_VIEWS);
    DFH_REQUIRE(f->depth_dtype == DFH_F32 || f->depth_dtype == DFH_F64, "%s: bad depth_dtype", what);
    DFH_REQUIRE(!fused || f->depth_dtype == DFH_F32, "%s: the fused association needs float32 depth maps", what);
    DFH_REQUIRE(f->H >= 2 && f->W >= 2 && f->scale != 0.0, "%s: bad depth map / scale", what);
    return DFH_OK;
}

// ... and of its normal gate
inline int check_gate(const char *what, const dfh_gn_normal_gate *g) {
    DFH_REQUIRE(g, "%s: null normal gate", what);
    DFH_REQUIRE(g->normals, "%s: null normal maps", what);
    DFH_REQUIRE(g->min_cos >= 0.0 && g->min_cos <= 1.0, "%s: min_cos %g outside [0, 1]", what, g->min_cos);      // (NaN fails)
    return DFH_OK;
}

// The association's kernel arguments.  cull: drop, per tile, the views none of its samples can be valid in (tile_view_mask):
// it costs a tile one barrier and one memory round trip (+5 % on the 3-view frame, where the views all face the object and
// nothing is dropped), so it is taken from four views up (the 8-view orbit: -9 % of the solve stage).
inline AssocArgs assoc_args(const dfh_gn_problem &p, const dfh_gn_frame &f, bool cull) {
    AssocArgs aa;
    for (int i = 0; i < 9; ++i) { aa.ap.K.m[i] = f.K[i]; aa.ap.Kinv.m[i] = f.Kinv[i]; }
    for (int i = 0; i < 8; ++i) aa.ap.lw.q[i] = p.lw_dq[i];
    aa.ap.scale = f.scale; aa.ap.inv_scale = 1.0 / f.scale;
    aa.ap.cx = f.center[0]; aa.ap.cy = f.center[1]; aa.ap.cz = f.center[2]; aa.ap.half = f.half; aa.ap.max_dist = f.max_dist;
    aa.ap.H = f.H; aa.ap.W = f.W; aa.ap.k = p.knn;
    aa.views = static_cast<const AssocView *>(f.views);
    aa.n_views = f.n_views;
    aa.cull = cull && f.n_views >= 4 && !on(opt().gn_no_view_cull) ? 1 : 0;
    return aa;
}
// What the sparse terms' checks share (a NaN fails every comparison it meets).  `term` / `item` are the nouns of the messages:
// "landmark" / "landmark", "photometric" / "photo sample".  First the scalars ...
inline int check_term_scalars(const char *what, const char *term, const char *item, int n, double weight, double huber) {
    DFH_REQUIRE(n >= 0, "%s: negative %s count", what, item);
    DFH_REQUIRE(weight >= 0.0 && weight < __builtin_huge_val(), "%s: %s weight negative or not finite", what, term);
    DFH_REQUIRE(huber >= 0.0, "%s: %s huber_delta negative or NaN", what, term);
    return DFH_OK;
}
// ... and after the term's own checks, in the order they have always been reported in, the arrays of a term with items: `items`,
// whether the item arrays are all there, and the plan of T = dfh_gn_landmarks / dfh_gn_photometric.
template <typename T>
inline int check_term_arrays(const char *what, const char *term, const char *item, const T *t, bool items) {
    if (t->n > 0) {
        DFH_REQUIRE(items, "%s: null %s pointer", what, item);
        DFH_REQUIRE(t->n_rows >= 1 && t->run_id && t->partial && t->blk_ptr && t->blk_ent && t->node_ptr && t->node_ent,
                    "%s: null %s plan array", what, term);
    }
    return DFH_OK;
}

// ... and of a landmark term (dfh_gn_landmarks)
inline int check_landmarks(const char *what, const dfh_gn_landmarks *l) {
    DFH_REQUIRE(l, "%s: null landmarks", what);
    const int rc = check_term_scalars(what, "landmark", "landmark", l->n, l->weight, l->huber_delta);
    if (rc != DFH_OK) return rc;
    DFH_REQUIRE(l->max_dist == l->max_dist, "%s: landmark max_dist is NaN", what);
    return check_term_arrays(what, "landmark", "landmark", l, l->pos && l->nbr && l->weights && l->target);
}

// The launch of gn_gather_kernel<knn> (dfh_solve.hip) for callers outside that file: the rows of `partial` (live flags behind the
// per-tile {cost, count} pairs `cc`) summed through the lists into vals / rhs / cost_count; no regulariser lists, every part.
int gn_gather_launch(int knn, const double *partial, const double *live, int n_rows, const int *blk_ptr, const int *blk_ent, int n_blocks,
                     const int *node_ptr, const int *node_ent, int n_nodes, double *vals, double *rhs, double *cost_count, const double *cc,
                     int n_cc, bool accumulate, const int *upper, int n_upper, void *stream);

// The landmark term added to the problem's system (dfh_landmarks.hip); both structs are checked by the caller.
int gn_add_landmarks_impl(const dfh_gn_problem &q, const dfh_gn_landmarks &l, void *stream);

// ... and of a photometric term with its frame (dfh_gn_photometric; `fused`: the frame also feeds a fused build)
inline int check_photometric(const char *what, const dfh_gn_photometric *t, const dfh_gn_frame *f, bool fused) {
    DFH_REQUIRE(t, "%s: null photometric term", what);
    int rc = check_frame(what, f, fused);
    if (rc == DFH_OK) rc = check_term_scalars(what, "photometric", "photo sample", t->n, t->weight, t->huber_delta);
    if (rc != DFH_OK) return rc;
    DFH_REQUIRE(t->max_diff == t->max_diff, "%s: photometric max_diff is NaN", what);
    DFH_REQUIRE(t->band_sd > 0.0, "%s: photometric band_sd must be > 0", what);
    DFH_REQUIRE(t->color, "%s: null colour image array", what);
    for (int v = 0; v < f->n_views; ++v) DFH_REQUIRE(t->color[v], "%s: colour image %d is null", what, v);
    return check_term_arrays(what, "photometric", "photo sample", t, t->pos && t->nbr && t->weights && t->ref);
}

// The photometric term added to the problem's system (dfh_photometric.hip); the structs are checked by the caller.
int gn_add_photometric_impl(const dfh_gn_problem &q, const dfh_gn_frame &f, const dfh_gn_photometric &t, void *stream);

inline GatedAssocArgs gated_assoc_args(const dfh_gn_problem &p, const dfh_gn_frame &f, const dfh_gn_normal_gate &g, bool cull) {
    GatedAssocArgs ga;
    static_cast<AssocArgs &>(ga) = assoc_args(p, f, cull);
    ga.ng = NormalGate{g.normals, g.min_cos};
    return ga;
}

}  // namespace dfh
