// K12 depth preprocessing (include/dfusion_hip.h: dfh_depth_prep): bilateral filter, vertex / normal map and flying-pixel mask of
// every depth map of a frame in ONE kernel and one launch.  float32 throughout, one rounding per operation (the build passes
// -ffp-contract=off; division and square root are the IEEE ones), in the header's operation order: tests/depth_prep_np.py restates
// it in numpy and the outputs agree bit for bit.
//
// A workgroup of 256 threads owns a tile of kDpTH x kDpTW = 16 x 64 output pixels of one view (grid: tiles_x, tiles_y, view):
//   1. the raw tile plus a halo of r + 1 pixels goes to LDS, lanes along x (row-contiguous loads); a pixel outside the image or
//      without a measurement is stored as +inf, which no tap test accepts ((inf - d)^2 * s is inf or NaN, never < n_lut) and no
//      centre test either (valid <=> value < 0 once the -inf / NaN inputs are gone);
//   2. the filtered value F of the tile plus a ONE-pixel halo (18 x 66) goes to LDS: the normals need F at the four neighbours;
//   3. every thread takes four pixels of the tile: neighbour tests, vertices, normal, mask, stores.
// range_lut and spatial sit in LDS too (the LUT read is a gather; the spatial weight is one broadcast read per tap).
// Row pitches are odd (raw: RW | 1, F: 67 dwords), so that a wave whose lanes straddle two tile rows in step 2 still reads
// distinct banks.  The 12-byte normals leave either as three strided dword stores per lane (RELAY = false) or re-laid through
// LDS (the raw tile's space, dead after step 2) into runs of consecutive dwords (RELAY = true); option k12_store picks.
#include <cmath>

#include "dfh_common.h"

namespace dfh {

constexpr int kDpTH = 16, kDpTW = 64, kDpThreads = 256, kDpMaxViews = 16, kDpMaxRadius = 8, kDpMaxLut = 4096;
constexpr int kDpFH = kDpTH + 2, kDpFW = kDpTW + 2, kDpFP = kDpFW | 1;       // the filtered tile with its one-pixel halo
constexpr int kDpRelay = kDpTH * kDpTW * 3;                                   // floats of a tile's normals

struct DpMaps { const void *d[kDpMaxViews]; };
struct DpParams {
    int H, W, r, n_lut, mask;
    float s, J, m2, nlf;              // range_scale, max_jump, min_cos^2, (float)n_lut
    float Kf[9];
};

__host__ __device__ inline int dp_raw_pitch(int r) { return (kDpTW + 2 * (r + 1)) | 1; }
__host__ __device__ inline int dp_raw_floats(int r, bool relay) {
    const int n = (kDpTH + 2 * (r + 1)) * dp_raw_pitch(r);
    return relay && n < kDpRelay ? kDpRelay : n;
}
static size_t dp_lds_bytes(int r, int n_lut, bool relay) {
    const int tables = r > 0 ? n_lut + (2 * r + 1) * (2 * r + 1) : 0;
    return sizeof(float) * (size_t)(tables + dp_raw_floats(r, relay) + kDpFH * kDpFP);
}

__device__ inline bool dp_valid(float d) { return d < 0.0f && d > -INFINITY; }

template <typename DepthT, bool RELAY>
__global__ __launch_bounds__(kDpThreads) void depth_prep_kernel(DpMaps maps, DpParams p, const float *__restrict__ spatial,
                                                                const float *__restrict__ range_lut, float *__restrict__ clean,
                                                                float *__restrict__ normals) {
    extern __shared__ float dp_lds[];
    const int r = p.r, halo = r + 1, H = p.H, W = p.W;
    const int RW = kDpTW + 2 * halo, RH = kDpTH + 2 * halo, RP = dp_raw_pitch(r);
    const int side = 2 * r + 1;
    const int n_lut = r > 0 ? p.n_lut : 0, n_sp = r > 0 ? side * side : 0;
    float *lut = dp_lds, *sp = lut + n_lut, *raw = sp + n_sp, *Ft = raw + dp_raw_floats(r, RELAY);
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kDpTW, y0 = blockIdx.y * kDpTH, view = blockIdx.z;
    const DepthT *__restrict__ D = static_cast<const DepthT *>(maps.d[view]);

    // ---- 1. raw tile + halo, tables -----------------------------------------------------------------------------------------
    for (int i = tid; i < RH * RW; i += kDpThreads) {
        const int ry = i / RW, rx = i - ry * RW;
        const int gy = y0 - halo + ry, gx = x0 - halo + rx;
        float e = INFINITY;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float t = (float)D[(size_t)gy * W + gx];
            if (dp_valid(t)) e = t;
        }
        raw[ry * RP + rx] = e;
    }
    for (int i = tid; i < n_lut; i += kDpThreads) lut[i] = range_lut[i];
    for (int i = tid; i < n_sp; i += kDpThreads) sp[i] = spatial[i];
    __syncthreads();

    // ---- 2. F on the tile + one pixel ---------------------------------------------------------------------------------------
    for (int i = tid; i < kDpFH * kDpFW; i += kDpThreads) {
        const int fy = i / kDpFW, fx = i - fy * kDpFW;
        const float *c = raw + (fy + r) * RP + (fx + r);            // F pixel (y0 - 1 + fy, x0 - 1 + fx) in raw coordinates
        const float d = *c;
        float F = 0.0f;
        if (d < 0.0f) {
            if (r == 0) {
                F = d;
            } else {
                float num = 0.0f, den = 0.0f;
                const float *w_sp = sp;
                for (int dy = -r; dy <= r; ++dy) {
                    const float *row = c + dy * RP;
                    for (int dx = -r; dx <= r; ++dx) {
                        const float e = row[dx];
                        const float delta = e - d;
                        const float q = (delta * delta) * p.s;
                        const bool ok = q < p.nlf;
                        const int idx = ok ? (int)q : 0;
                        const float w = *w_sp++ * lut[idx];
                        const float we = w * e;
                        num = num + (ok ? we : 0.0f);              // a tap that does not count is selected out: inf * 0 is NaN
                        den = den + (ok ? w : 0.0f);
                    }
                }
                F = den > 0.0f ? num / den : 0.0f;
            }
        }
        Ft[fy * kDpFP + fx] = F;
    }
    __syncthreads();

    // ---- 3. normals and mask: thread (tx, wy) takes rows wy*4 .. wy*4+3 at column tx ------------------------------------------
    const int tx = tid & (kDpTW - 1), wy = tid / kDpTW;
    const int gx = x0 + tx;
    const float xf = (float)gx, xl = (float)(gx - 1), xr = (float)(gx + 1);
    const float *Kf = p.Kf;
#pragma unroll
    for (int k = 0; k < kDpTH / (kDpThreads / kDpTW); ++k) {
        const int ly = wy * (kDpTH / (kDpThreads / kDpTW)) + k, gy = y0 + ly;
        const bool inside = gy < H && gx < W;
        const float *fc = Ft + (ly + 1) * kDpFP + (tx + 1);
        const float Fc = *fc;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        bool has = false;
        if (inside && dp_valid(Fc)) {
            const float Fl = fc[-1], Fr = fc[1], Fu = fc[-kDpFP], Fd = fc[kDpFP];
            if (dp_valid(Fl) && dp_valid(Fr) && dp_valid(Fu) && dp_valid(Fd) && fabsf(Fl - Fc) <= p.J && fabsf(Fr - Fc) <= p.J &&
                fabsf(Fu - Fc) <= p.J && fabsf(Fd - Fc) <= p.J) {
                const float yf = (float)gy, yu = (float)(gy - 1), yd = (float)(gy + 1);
                float P[3], a[3], b[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float k0 = Kf[3 * i], k1 = Kf[3 * i + 1], k2 = Kf[3 * i + 2];
                    P[i] = -Fc * ((k0 * xf + k1 * yf) + k2);
                    const float Pr = -Fr * ((k0 * xr + k1 * yf) + k2), Pl = -Fl * ((k0 * xl + k1 * yf) + k2);
                    const float Pd = -Fd * ((k0 * xf + k1 * yd) + k2), Pu = -Fu * ((k0 * xf + k1 * yu) + k2);
                    a[i] = Pr - Pl;
                    b[i] = Pd - Pu;
                }
                const float n0 = a[1] * b[2] - a[2] * b[1];
                const float n1 = a[2] * b[0] - a[0] * b[2];
                const float n2 = a[0] * b[1] - a[1] * b[0];
                const float l2 = (n0 * n0 + n1 * n1) + n2 * n2;
                if (l2 > 0.0f && l2 < INFINITY) {
                    const float len = sqrtf(l2);
                    float h0 = n0 / len, h1 = n1 / len, h2 = n2 / len;
                    float c = (h0 * P[0] + h1 * P[1]) + h2 * P[2];
                    if (c > 0.0f) { h0 = -h0; h1 = -h1; h2 = -h2; c = -c; }
                    const float pp = (P[0] * P[0] + P[1] * P[1]) + P[2] * P[2];
                    if (c * c >= p.m2 * pp) { has = true; nx = h0; ny = h1; nz = h2; }
                }
            }
        }
        const size_t pix = ((size_t)view * H + (inside ? gy : 0)) * W + (inside ? gx : 0);
        if (clean && inside) clean[pix] = (p.mask == 0 || has) ? Fc : 0.0f;
        if (normals) {
            if (RELAY) {                                             // (raw is dead: every thread is past the barrier after step 2)
                float *o = raw + (ly * kDpTW + tx) * 3;
                o[0] = nx; o[1] = ny; o[2] = nz;
            } else if (inside) {
                float *o = normals + pix * 3;
                o[0] = nx; o[1] = ny; o[2] = nz;
            }
        }
    }
    if (RELAY && normals) {                                          // (uniform: the barrier is reached by all or by none)
        __syncthreads();
        const int cols = W - x0 < kDpTW ? W - x0 : kDpTW, run = cols * 3;
        for (int ly = wy; ly < kDpTH; ly += kDpThreads / kDpTW) {
            const int gy = y0 + ly;
            if (gy >= H) break;
            float *o = normals + (((size_t)view * H + gy) * W + x0) * 3;
            const float *src = raw + ly * kDpTW * 3;
            for (int j = tx; j < run; j += kDpTW) o[j] = src[j];
        }
    }
}

template <typename DepthT>
static int launch_depth_prep(const DpMaps &maps, const DpParams &p, int n_views, const float *spatial, const float *range_lut, float *clean,
                             float *normals, bool relay, hipStream_t s) {
    const dim3 grid((unsigned)((p.W + kDpTW - 1) / kDpTW), (unsigned)((p.H + kDpTH - 1) / kDpTH), (unsigned)n_views);
    const size_t lds = dp_lds_bytes(p.r, p.n_lut, relay);
    if (relay)
        hipLaunchKernelGGL((depth_prep_kernel<DepthT, true>), grid, dim3(kDpThreads), lds, s, maps, p, spatial, range_lut, clean, normals);
    else
        hipLaunchKernelGGL((depth_prep_kernel<DepthT, false>), grid, dim3(kDpThreads), lds, s, maps, p, spatial, range_lut, clean, normals);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

}  // namespace dfh

extern "C" int dfh_depth_prep_tile(int tile_hw[2]) {
    using namespace dfh;
    DFH_REQUIRE(tile_hw, "dfh_depth_prep_tile: null pointer");
    tile_hw[0] = kDpTH;
    tile_hw[1] = kDpTW;
    return DFH_OK;
}

extern "C" int dfh_depth_prep(const dfh_depth_prep_params *q, float *clean, float *normals, void *stream) {
    using namespace dfh;
    static const char *const me = "dfh_depth_prep";
    DFH_REQUIRE(q, "%s: null params", me);
    DFH_REQUIRE(q->n_views >= 1 && q->n_views <= kDpMaxViews, "%s: %d views (1..%d per call)", me, q->n_views, kDpMaxViews);
    DFH_REQUIRE(q->depth, "%s: null depth array", me);
    DFH_REQUIRE(q->depth_dtype == DFH_F32 || q->depth_dtype == DFH_F64, "%s: bad depth_dtype %d", me, q->depth_dtype);
    DFH_REQUIRE(q->H >= 2 && q->W >= 2 && (long)q->H * q->W < (1L << 31), "%s: bad depth map size %dx%d", me, q->H, q->W);
    DFH_REQUIRE(q->radius >= 0 && q->radius <= kDpMaxRadius, "%s: radius %d outside [0,%d]", me, q->radius, kDpMaxRadius);
    DFH_REQUIRE(q->radius == 0 || (q->spatial && q->range_lut), "%s: null spatial / range_lut table with radius %d", me, q->radius);
    DFH_REQUIRE(q->n_lut >= 1 && q->n_lut <= kDpMaxLut, "%s: n_lut %d outside [1,%d]", me, q->n_lut, kDpMaxLut);
    DFH_REQUIRE(std::isfinite(q->range_scale) && q->range_scale > 0.0, "%s: range_scale %g is not finite and > 0", me, q->range_scale);
    DFH_REQUIRE(std::isfinite(q->max_jump) && q->max_jump >= 0.0, "%s: max_jump %g is not finite and >= 0", me, q->max_jump);
    DFH_REQUIRE(q->min_cos >= 0.0 && q->min_cos <= 1.0, "%s: min_cos %g outside [0,1]", me, q->min_cos);
    DFH_REQUIRE(q->mask == 0 || q->mask == 1, "%s: mask %d is not 0 or 1", me, q->mask);
    DFH_REQUIRE(clean || normals, "%s: both outputs are null", me);
    DpMaps maps = {};
    for (int v = 0; v < q->n_views; ++v) {
        DFH_REQUIRE(q->depth[v], "%s: depth map %d is null", me, v);
        DFH_REQUIRE(q->depth[v] != (const void *)clean && q->depth[v] != (const void *)normals,
                    "%s: depth map %d is also an output (in-place use is not supported)", me, v);
        maps.d[v] = q->depth[v];
    }
    DpParams p = {};
    p.H = q->H; p.W = q->W; p.r = q->radius; p.n_lut = q->n_lut; p.mask = q->mask;
    p.s = (float)q->range_scale;
    p.J = (float)q->max_jump;
    const float mc = (float)q->min_cos;
    p.m2 = mc * mc;
    p.nlf = (float)q->n_lut;
    for (int i = 0; i < 9; ++i) p.Kf[i] = (float)q->Kinv[i];
    const bool relay = opt().k12_store == 1;          // unset: the strided stores, the faster layout at every size measured (DESIGN: K12)
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (q->depth_dtype == DFH_F32) return launch_depth_prep<float>(maps, p, q->n_views, q->spatial, q->range_lut, clean, normals, relay, s);
    return launch_depth_prep<double>(maps, p, q->n_views, q->spatial, q->range_lut, clean, normals, relay, s);
}
