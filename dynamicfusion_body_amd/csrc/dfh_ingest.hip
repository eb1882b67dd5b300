// K19 RGB-D ingest (include/dfusion_hip.h: dfh_rgbd_ingest): raw uint16 depth maps with lens distortion and per-camera intrinsics,
// and the raw images of a second (colour) camera, become the frame inputs every other entry point reads -- undistorted negative
// depth maps through ONE pinhole, and colour registered to the depth pixels with an occlusion test.  fp64 throughout, one rounding
// per operation (the build passes -ffp-contract=off; division, rint and floor are the IEEE ones), in the header's operation order:
// tests/ingest_np.py restates it in numpy and all outputs, the z-buffer included, agree bit for bit.
//
// Three launches, all views in each (grid: tiles_x, tiles_y, view), one thread per OUTPUT depth pixel, a workgroup of 256 threads
// on a tile of kIgTH x kIgTW = 4 x 64 pixels (lanes along x: a wave stores one 256-byte row segment):
//   rectify  A: decode + undistort -> depth_out.  It also clears the z-buffer (grid-stride dword stores of 0xffffffff) and writes
//            the views' depth-side calibration records from its kernel arguments into the workspace's table.
//   splat    B: every valid pixel projects its centre and two corners into the colour camera and atomicMin's the centre's depth
//            key (the bits of a positive float32 order as unsigned integers) over the clipped rectangle.  It writes the views'
//            colour-side records into the table.
//   gather   C: every valid pixel projects its centre again, compares its key with the z-buffer and samples the colour image.
// The calibration is 30 doubles per view: sixteen views do not fit one 4 KB kernel-argument block, so each half travels as
// kernel arguments of the launch BEFORE the first one that reads it from memory (rectify carries the depth side, 1.3 KB, and uses
// it in place; splat carries the colour side, 2.8 KB), and nothing is copied from the host.  The table is indexed by blockIdx.z
// only: uniform addresses.  A, B and C each recompute the pixel's source lookup (a 2-byte gather and ~40 fp64 operations)
// instead of passing z through memory: float32 depth_out has lost the bits B and C need.
// No LDS, no private arrays; the splat's loop is bounded by max_splat <= 16 in each direction.
#include <cmath>
#include <cstdint>

#include "dfh_common.h"

namespace dfh {

constexpr int kIgTH = 4, kIgTW = 64, kIgThreads = kIgTH * kIgTW, kIgMaxViews = 16, kIgMaxSplat = 16;

struct IgDepthSide { double f[4], k[5], ident; };                 // fx fy cx cy | k1 k2 p1 p2 k3 | 1: all five are 0 (distort is skipped)
struct IgColorSide { double f[4], k[5], T[12], ident; };
static_assert(sizeof(IgDepthSide) == 80 && sizeof(IgColorSide) == 176, "calibration records are 10 and 22 doubles");
struct IgDepthTable { IgDepthSide v[kIgMaxViews]; };
struct IgColorTable { IgColorSide v[kIgMaxViews]; };
struct IgPtrs { const void *p[kIgMaxViews]; };
struct IgParams {
    int Hd, Wd, Hc, Wc, C, max_splat, sample, pad;
    double fx, fy, cx, cy, depth_scale, z_min, z_max, occl_tol;
};
// the workspace: the z-buffer (n_views x Hc x Wc uint32), then -- 256-byte aligned -- the depth-side and the colour-side records
constexpr size_t kIgTableBytes = sizeof(IgDepthTable) + sizeof(IgColorTable);
static size_t ig_table_offset(int n_views, int Hc, int Wc) { return ((size_t)4 * n_views * Hc * Wc + 255) / 256 * 256; }

__device__ inline void ig_distort(double x, double y, const double *k, double &xd, double &yd) {
    const double r2 = x * x + y * y;
    const double rad = 1.0 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]));
    xd = x * rad + (2.0 * k[2] * (x * y) + k[3] * (r2 + 2.0 * (x * x)));
    yd = y * rad + (k[2] * (r2 + 2.0 * (y * y)) + 2.0 * k[3] * (x * y));
}

// Stage A, steps 1-6 for output pixel (i, j): true = valid; z = (double)raw * depth_scale; (x, y) = the pixel's ideal coordinates
__device__ inline bool ig_decode(const IgParams &p, const IgDepthSide &d, const unsigned short *__restrict__ raw, int i, int j, double &x,
                                 double &y, double &z) {
    x = ((double)i - p.cx) / p.fx;
    y = ((double)j - p.cy) / p.fy;
    double xd = x, yd = y;
    if (d.ident == 0.0) ig_distort(x, y, d.k, xd, yd);
    const double us = d.f[0] * xd + d.f[2], vs = d.f[1] * yd + d.f[3];
    const double si = rint(us), sj = rint(vs);
    const bool inside = si >= 0.0 && si <= (double)(p.Wd - 1) && sj >= 0.0 && sj <= (double)(p.Hd - 1);      // (a NaN fails)
    unsigned r = 0;
    if (inside) r = raw[(size_t)(int)sj * p.Wd + (int)si];
    z = (double)r * p.depth_scale;
    return inside && r != 0 && z >= p.z_min && (p.z_max <= 0.0 || z <= p.z_max);
}

// Stage B, steps 1-6 for the point with ideal coordinates (x, y) and depth z: false = not in front of the colour camera
__device__ inline bool ig_project(const IgColorSide &c, double x, double y, double z, double &u, double &v, double &w) {
    const double P0 = x * z, P1 = y * z;
    const double q0 = ((c.T[0] * P0 + c.T[1] * P1) + c.T[2] * z) + c.T[3];
    const double q1 = ((c.T[4] * P0 + c.T[5] * P1) + c.T[6] * z) + c.T[7];
    const double q2 = ((c.T[8] * P0 + c.T[9] * P1) + c.T[10] * z) + c.T[11];
    w = q2;
    u = v = 0.0;
    if (!(q2 > 0.0)) return false;
    const double xc = q0 / q2, yc = q1 / q2;
    double xd = xc, yd = yc;
    if (c.ident == 0.0) ig_distort(xc, yc, c.k, xd, yd);
    u = c.f[0] * xd + c.f[2];
    v = c.f[1] * yd + c.f[3];
    return true;
}

__global__ __launch_bounds__(kIgThreads) void ingest_rectify_kernel(IgPtrs raw, IgParams p, IgDepthTable tab, float *__restrict__ depth_out,
                                                                    unsigned *__restrict__ zbuf, size_t n_zbuf, IgDepthSide *__restrict__ dtab_out) {
    const int view = blockIdx.z;
    const size_t n_threads = (size_t)gridDim.x * gridDim.y * gridDim.z * kIgThreads;
    const size_t lin = (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kIgThreads + threadIdx.x;
    for (size_t k = lin; k < n_zbuf; k += n_threads) zbuf[k] = 0xffffffffu;
    if (dtab_out && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < sizeof(IgDepthSide) / 8)
        reinterpret_cast<double *>(dtab_out + view)[threadIdx.x] = reinterpret_cast<const double *>(&tab.v[view])[threadIdx.x];
    const int i = blockIdx.x * kIgTW + (threadIdx.x % kIgTW), j = blockIdx.y * kIgTH + (threadIdx.x / kIgTW);
    if (i >= p.Wd || j >= p.Hd) return;
    double x, y, z;
    const bool valid = ig_decode(p, tab.v[view], static_cast<const unsigned short *>(raw.p[view]), i, j, x, y, z);
    depth_out[((size_t)view * p.Hd + j) * p.Wd + i] = valid ? (float)(-z) : 0.0f;
}

__global__ __launch_bounds__(kIgThreads) void ingest_splat_kernel(IgPtrs raw, IgParams p, IgColorTable tab, const IgDepthSide *__restrict__ dtab,
                                                                  IgColorSide *__restrict__ ctab_out, unsigned *__restrict__ zbuf) {
    const int view = blockIdx.z;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < sizeof(IgColorSide) / 8)
        reinterpret_cast<double *>(ctab_out + view)[threadIdx.x] = reinterpret_cast<const double *>(&tab.v[view])[threadIdx.x];
    const int i = blockIdx.x * kIgTW + (threadIdx.x % kIgTW), j = blockIdx.y * kIgTH + (threadIdx.x / kIgTW);
    if (i >= p.Wd || j >= p.Hd) return;
    double x, y, z;
    if (!ig_decode(p, dtab[view], static_cast<const unsigned short *>(raw.p[view]), i, j, x, y, z)) return;
    const IgColorSide &c = tab.v[view];
    double u0, v0, w0, u1, v1, w1, u2, v2, w2;
    const bool f0 = ig_project(c, x, y, z, u0, v0, w0);                 // (the centre's ideal coordinates are A's: the same expressions)
    const bool f1 = ig_project(c, (((double)i - 0.5) - p.cx) / p.fx, (((double)j - 0.5) - p.cy) / p.fy, z, u1, v1, w1);
    const bool f2 = ig_project(c, (((double)i + 0.5) - p.cx) / p.fx, (((double)j + 0.5) - p.cy) / p.fy, z, u2, v2, w2);
    if (!(f0 && f1 && f2)) return;
    if (!(__builtin_isfinite(u1) && __builtin_isfinite(u2) && __builtin_isfinite(v1) && __builtin_isfinite(v2))) return;
    double a0 = rint(fmin(u1, u2)), a1 = rint(fmax(u1, u2)), b0 = rint(fmin(v1, v2)), b1 = rint(fmax(v1, v2));
    a0 = fmax(a0, 0.0);                                   // clipped to the image, then cut to max_splat columns and rows: all on
    b0 = fmax(b0, 0.0);                                   // doubles, so that a far-off rectangle never goes through an int
    a1 = fmin(fmin(a1, (double)(p.Wc - 1)), a0 + (double)(p.max_splat - 1));
    b1 = fmin(fmin(b1, (double)(p.Hc - 1)), b0 + (double)(p.max_splat - 1));
    if (!(a0 <= a1 && b0 <= b1)) return;
    const unsigned key = __float_as_uint((float)w0);
    unsigned *zb = zbuf + (size_t)view * p.Hc * p.Wc;
    const int c0 = (int)a0, c1 = (int)a1, r0 = (int)b0, r1 = (int)b1;         // 0 <= c0 <= c1 <= Wc-1, 0 <= r0 <= r1 <= Hc-1
    for (int r = r0; r <= r1; ++r)
        for (int cc = c0; cc <= c1; ++cc) atomicMin(zb + (size_t)r * p.Wc + cc, key);
}

// one colour tap as three doubles (C == 4: one dword load)
__device__ inline void ig_tap(const unsigned char *__restrict__ img, size_t pix, int C, double &r, double &g, double &b) {
    if (C == 4) {
        const unsigned t = reinterpret_cast<const unsigned *>(img)[pix];
        r = (double)(t & 255u); g = (double)((t >> 8) & 255u); b = (double)((t >> 16) & 255u);
    } else {
        const unsigned char *q = img + pix * 3;
        r = (double)q[0]; g = (double)q[1]; b = (double)q[2];
    }
}

__device__ inline unsigned ig_bilerp(double fu, double fv, double c00, double c10, double c01, double c11) {
    const double c = (1.0 - fv) * ((1.0 - fu) * c00 + fu * c10) + fv * ((1.0 - fu) * c01 + fu * c11);
    return (unsigned)(int)rint(c);
}

__global__ __launch_bounds__(kIgThreads) void ingest_gather_kernel(IgPtrs raw, IgPtrs color, IgParams p, const IgDepthSide *__restrict__ dtab,
                                                                   const IgColorSide *__restrict__ ctab, const unsigned *__restrict__ zbuf,
                                                                   unsigned *__restrict__ color_out, float *__restrict__ color_depth_out) {
    const int view = blockIdx.z;
    const int i = blockIdx.x * kIgTW + (threadIdx.x % kIgTW), j = blockIdx.y * kIgTH + (threadIdx.x / kIgTW);
    if (i >= p.Wd || j >= p.Hd) return;
    double x, y, z, u, v, w;
    unsigned rgbx = 0;
    if (ig_decode(p, dtab[view], static_cast<const unsigned short *>(raw.p[view]), i, j, x, y, z) &&
        ig_project(ctab[view], x, y, z, u, v, w) &&
        u >= 0.0 && u < (double)(p.Wc - 1) && v >= 0.0 && v < (double)(p.Hc - 1)) {                      // (a NaN fails)
        const int ru = (int)rint(u), rv = (int)rint(v);
        const float zb = __uint_as_float(zbuf[((size_t)view * p.Hc + rv) * p.Wc + ru]);
        if (!((double)zb + p.occl_tol < (double)(float)w)) {
            const unsigned char *img = static_cast<const unsigned char *>(color.p[view]);
            if (p.sample == 0) {
                double r, g, b;
                ig_tap(img, (size_t)rv * p.Wc + ru, p.C, r, g, b);
                rgbx = (unsigned)r | (unsigned)g << 8 | (unsigned)b << 16 | 255u << 24;
            } else {
                const double fi = floor(u), fj = floor(v), fu = u - fi, fv = v - fj;
                const size_t t = (size_t)(int)fj * p.Wc + (int)fi;
                double r00, g00, b00, r10, g10, b10, r01, g01, b01, r11, g11, b11;
                ig_tap(img, t, p.C, r00, g00, b00);
                ig_tap(img, t + 1, p.C, r10, g10, b10);
                ig_tap(img, t + p.Wc, p.C, r01, g01, b01);
                ig_tap(img, t + p.Wc + 1, p.C, r11, g11, b11);
                rgbx = ig_bilerp(fu, fv, r00, r10, r01, r11) | ig_bilerp(fu, fv, g00, g10, g01, g11) << 8 |
                       ig_bilerp(fu, fv, b00, b10, b01, b11) << 16 | 255u << 24;
            }
        }
    }
    const size_t pix = ((size_t)view * p.Hd + j) * p.Wd + i;
    color_out[pix] = rgbx;
    if (color_depth_out) color_depth_out[pix] = rgbx ? (float)(-z) : 0.0f;
}

static bool ig_finite(const double *a, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(a[i])) return false;
    return true;
}

static bool ig_zero(const double *a, int n) {
    for (int i = 0; i < n; ++i)
        if (a[i] != 0.0) return false;
    return true;
}

}  // namespace dfh

extern "C" int dfh_rgbd_ingest_tile(int tile_hw[2]) {
    using namespace dfh;
    DFH_REQUIRE(tile_hw, "dfh_rgbd_ingest_tile: null pointer");
    tile_hw[0] = kIgTH;
    tile_hw[1] = kIgTW;
    return DFH_OK;
}

extern "C" size_t dfh_rgbd_ingest_workspace_bytes(int n_views, int Hc, int Wc) {
    using namespace dfh;
    if (n_views < 1 || n_views > kIgMaxViews || Hc < 2 || Wc < 2 || (long)Hc * Wc >= (1L << 31)) return 0;
    return ig_table_offset(n_views, Hc, Wc) + kIgTableBytes;
}

extern "C" int dfh_rgbd_ingest(const dfh_rgbd_ingest_params *q, float *depth_out, void *color_out, float *color_depth_out, void *zbuf,
                               void *stream) {
    using namespace dfh;
    static const char *const me = "dfh_rgbd_ingest";
    DFH_REQUIRE(q, "%s: null params", me);
    DFH_REQUIRE(q->n_views >= 1 && q->n_views <= kIgMaxViews, "%s: %d views (1..%d per call)", me, q->n_views, kIgMaxViews);
    DFH_REQUIRE(q->raw_depth && q->views, "%s: null raw_depth / views array", me);
    DFH_REQUIRE(q->Hd >= 2 && q->Wd >= 2 && (long)q->Hd * q->Wd < (1L << 31), "%s: bad depth map size %dx%d", me, q->Hd, q->Wd);
    const bool colour = q->raw_color != nullptr;
    if (colour) {
        DFH_REQUIRE(q->Hc >= 2 && q->Wc >= 2 && (long)q->Hc * q->Wc < (1L << 31), "%s: bad colour image size %dx%d", me, q->Hc, q->Wc);
        DFH_REQUIRE(q->C == 3 || q->C == 4, "%s: %d colour channels (3 or 4)", me, q->C);
        DFH_REQUIRE(color_out && zbuf, "%s: colour images given without color_out / zbuf", me);
        DFH_REQUIRE(reinterpret_cast<uintptr_t>(zbuf) % 8 == 0, "%s: zbuf must be 8-byte aligned", me);
    }
    const double out_k[4] = {q->fx, q->fy, q->cx, q->cy};
    DFH_REQUIRE(ig_finite(out_k, 4) && q->fx > 0.0 && q->fy > 0.0, "%s: output intrinsics are not finite with fx, fy > 0", me);
    DFH_REQUIRE(std::isfinite(q->depth_scale) && q->depth_scale > 0.0, "%s: depth_scale %g is not finite and > 0", me, q->depth_scale);
    DFH_REQUIRE(!std::isnan(q->z_min) && !std::isnan(q->z_max), "%s: z_min / z_max is NaN", me);
    DFH_REQUIRE(q->occl_tol >= 0.0, "%s: occl_tol %g is negative or NaN", me, q->occl_tol);
    DFH_REQUIRE(q->max_splat >= 1 && q->max_splat <= kIgMaxSplat, "%s: max_splat %d outside [1,%d]", me, q->max_splat, kIgMaxSplat);
    DFH_REQUIRE(q->sample == 0 || q->sample == 1, "%s: sample %d is not 0 (nearest) or 1 (bilinear)", me, q->sample);
    DFH_REQUIRE(depth_out, "%s: null depth_out", me);
    IgPtrs raw = {}, col = {};
    IgDepthTable dt = {};
    IgColorTable ct = {};
    for (int v = 0; v < q->n_views; ++v) {
        const dfh_rgbd_view &c = q->views[v];
        DFH_REQUIRE(q->raw_depth[v], "%s: raw depth map %d is null", me, v);
        DFH_REQUIRE(!colour || q->raw_color[v], "%s: raw colour image %d is null", me, v);
        DFH_REQUIRE(!colour || q->C != 4 || reinterpret_cast<uintptr_t>(q->raw_color[v]) % 4 == 0,
                    "%s: 4-channel colour image %d is not 4-byte aligned", me, v);
        DFH_REQUIRE(ig_finite(c.fd, 4) && ig_finite(c.kd, 5) && ig_finite(c.fc, 4) && ig_finite(c.kc, 5) && ig_finite(c.T_dc, 12),
                    "%s: view %d has a non-finite calibration value", me, v);
        DFH_REQUIRE(c.fd[0] > 0.0 && c.fd[1] > 0.0, "%s: view %d: depth camera fx, fy must be > 0", me, v);
        DFH_REQUIRE(!colour || (c.fc[0] > 0.0 && c.fc[1] > 0.0), "%s: view %d: colour camera fx, fy must be > 0", me, v);
        raw.p[v] = q->raw_depth[v];
        if (colour) col.p[v] = q->raw_color[v];
        for (int i = 0; i < 4; ++i) { dt.v[v].f[i] = c.fd[i]; ct.v[v].f[i] = c.fc[i]; }
        for (int i = 0; i < 5; ++i) { dt.v[v].k[i] = c.kd[i]; ct.v[v].k[i] = c.kc[i]; }
        for (int i = 0; i < 12; ++i) ct.v[v].T[i] = c.T_dc[i];
        dt.v[v].ident = ig_zero(c.kd, 5) ? 1.0 : 0.0;
        ct.v[v].ident = ig_zero(c.kc, 5) ? 1.0 : 0.0;
    }
    IgParams p = {};
    p.Hd = q->Hd; p.Wd = q->Wd; p.max_splat = q->max_splat; p.sample = q->sample;
    if (colour) { p.Hc = q->Hc; p.Wc = q->Wc; p.C = q->C; }
    p.fx = q->fx; p.fy = q->fy; p.cx = q->cx; p.cy = q->cy;
    p.depth_scale = q->depth_scale; p.z_min = q->z_min; p.z_max = q->z_max; p.occl_tol = q->occl_tol;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((p.Wd + kIgTW - 1) / kIgTW), (unsigned)((p.Hd + kIgTH - 1) / kIgTH), (unsigned)q->n_views);
    const size_t n_zbuf = colour ? (size_t)q->n_views * p.Hc * p.Wc : 0;
    unsigned *zb = static_cast<unsigned *>(zbuf);
    IgDepthSide *dtab = nullptr;
    IgColorSide *ctab = nullptr;
    if (colour) {
        char *t = static_cast<char *>(zbuf) + ig_table_offset(q->n_views, p.Hc, p.Wc);
        dtab = reinterpret_cast<IgDepthSide *>(t);
        ctab = reinterpret_cast<IgColorSide *>(t + sizeof(IgDepthTable));
    }
    hipLaunchKernelGGL(ingest_rectify_kernel, grid, dim3(kIgThreads), 0, s, raw, p, dt, depth_out, zb, n_zbuf, dtab);
    DFH_HIP_CHECK(hipGetLastError());
    if (!colour) return DFH_OK;
    hipLaunchKernelGGL(ingest_splat_kernel, grid, dim3(kIgThreads), 0, s, raw, p, ct, dtab, ctab, zb);
    DFH_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ingest_gather_kernel, grid, dim3(kIgThreads), 0, s, raw, col, p, dtab, ctab, zb, static_cast<unsigned *>(color_out),
                       color_depth_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}
