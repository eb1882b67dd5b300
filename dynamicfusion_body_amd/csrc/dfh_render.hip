// Multi-view triangle rasterizer: depth, face-id and normal maps of one triangle mesh in V views of H x W pixels, the
// "model-to-frame prediction" of DynamicFusion / KinectFusion.  No reference counterpart (the reference never renders its
// model); the semantics are stated in include/dfusion_hip.h (dfh_render_*) and restated in numpy by tests/render_np.py.
//
// Work decomposition (deterministic whatever the schedule: one 64-bit key per pixel, (float depth bits) << 32 | face,
// reduced with atomicMin -- the nearest surface wins, ties go to the lowest face id):
//   render_small_kernel   one lane per (triangle, view): projection, set-up, and a walk of the clamped bounding box when it
//                         holds at most kRenderSmallPixels pixels (marching-cubes meshes seen at about one voxel per pixel:
//                         triangles of a pixel or less); larger boxes are appended to a list
//   render_large_kernel   a fixed grid of workgroups pulls the listed (triangle, view) pairs; the 256 lanes of a workgroup
//                         tile the pair's box (a triangle covering the whole image is 256 pixels per lane-step, not one lane's
//                         million)
//   render_resolve_kernel one lane per pixel: the key -> depth (-z, the reference's storage convention) and face id; the
//                         normal is re-interpolated from the winning face (same arithmetic as the raster pass)
//   samples_*_kernel     the visible-surface samples (dfh_render_samples_*): see below, behind the resolve pass
//   render_vertex_ids_kernel  one lane per pixel: the key -> the winning face's vertex with the largest perspective-correct
//                         coordinate, and the depth as an 8-bit grey level (dfh_render_vertex_ids, K15): behind the samples
// Everything that decides coverage and depth runs in fp64 with -ffp-contract=off, so the numpy restatement with the same
// operation order gives the same bits.
#include "dfh_common.h"
#include "dfh_scan.h"

#include <cmath>

namespace dfh {

constexpr int kRenderBlock = 256;
constexpr int kRenderMaxViews = 16;
// Boxes up to 64 pixels (8 x 8) are walked by one lane.  A marching-cubes triangle at about one voxel per pixel has a box of
// 1-4 pixels, so a wave's lanes finish together; a lane that walks 64 pixels holds its wave for ~64 iterations, the price of
// the rare larger triangle without a second launch's list round trip.  Every box pixel that passes the edge test costs one
// 64-bit atomicMin to a scattered address.  The rate of 64-bit umin on gfx950 is not measured; for float adds with every lane
// on a different row MI355X_MICROARCH.md gives 0.08 TB/s, 17x below the coalesced rate, and that is the shape here.  A plain
// load of the key in front of the atomic skips it when the stored key is already smaller: keys only decrease, so a stale
// value can only be larger than the true one and the skip never loses a write.
constexpr int kRenderSmallPixels = 64;
constexpr unsigned long long kRenderEmpty = ~0ull;

struct RenderView {
    double k[5];              // K00 K01 K02 K11 K12
    double r[12];             // lw, 3 x 4 row-major (world -> camera)
};

struct RenderParams {
    int nv, H, W;
    long nverts, nfaces;
    double scale, half, center[3], znear;
    RenderView view[kRenderMaxViews];
};

// One triangle in one view after projection: screen positions, camera depths, area.
struct Tri {
    double u[3], v[3], z[3];
    double A;
    int x0, x1, y0, y1;       // clamped bounding box of pixel centres (inclusive)
};

__device__ __forceinline__ void render_project(const RenderParams &p, const RenderView &vw, const double *__restrict__ P, double &u,
                                               double &v, double &z) {
    const double w0 = p.scale * (P[0] - p.half) + p.center[0];
    const double w1 = p.scale * (P[1] - p.half) + p.center[1];
    const double w2 = p.scale * (P[2] - p.half) + p.center[2];
    const double *r = vw.r;
    const double c0 = r[0] * w0 + r[1] * w1 + r[2] * w2 + r[3];
    const double c1 = r[4] * w0 + r[5] * w1 + r[6] * w2 + r[7];
    const double c2 = r[8] * w0 + r[9] * w1 + r[10] * w2 + r[11];
    u = (vw.k[0] * c0 + vw.k[1] * c1 + vw.k[2] * c2) / c2;
    v = (vw.k[3] * c1 + vw.k[4] * c2) / c2;
    z = c2;
}

// Edge value of edge (a, b) at (x, y).  Evaluated from the lexicographically smaller end point (and negated when that is b),
// so the two triangles that share an edge get exactly opposite values and a closed mesh leaves no pixel uncovered.
__device__ __forceinline__ double render_edge(double ua, double va, double ub, double vb, double x, double y) {
    if (ua < ub || (ua == ub && va < vb)) return (x - ua) * (vb - va) - (y - va) * (ub - ua);
    return -((x - ub) * (va - vb) - (y - vb) * (ua - ub));
}

// false: the triangle draws nothing in this view (a vertex at c2 <= znear, a non-finite screen coordinate, zero or non-finite
// area, an empty clamped box, or a vertex index outside [0, nverts))
__device__ __forceinline__ bool render_setup(const RenderParams &p, const RenderView &vw, const double *__restrict__ verts,
                                             const int *__restrict__ faces, long f, Tri &t) {
    for (int i = 0; i < 3; ++i) {
        const int vi = faces[3 * f + i];
        if (vi < 0 || vi >= p.nverts) return false;
        render_project(p, vw, verts + 3 * (size_t)vi, t.u[i], t.v[i], t.z[i]);
        if (!(t.z[i] > p.znear) || !isfinite(t.u[i]) || !isfinite(t.v[i])) return false;
    }
    t.A = (t.u[2] - t.u[0]) * (t.v[1] - t.v[0]) - (t.v[2] - t.v[0]) * (t.u[1] - t.u[0]);
    if (!isfinite(t.A) || t.A == 0.0) return false;
    const double xl = fmax(0.0, ceil(fmin(fmin(t.u[0], t.u[1]), t.u[2])));
    const double xh = fmin((double)(p.W - 1), floor(fmax(fmax(t.u[0], t.u[1]), t.u[2])));
    const double yl = fmax(0.0, ceil(fmin(fmin(t.v[0], t.v[1]), t.v[2])));
    const double yh = fmin((double)(p.H - 1), floor(fmax(fmax(t.v[0], t.v[1]), t.v[2])));
    if (!(xl <= xh) || !(yl <= yh)) return false;
    t.x0 = (int)xl; t.x1 = (int)xh; t.y0 = (int)yl; t.y1 = (int)yh;
    return true;
}

// Barycentric weights (edge value / A) at pixel (x, y); false if the pixel is not covered.
__device__ __forceinline__ bool render_bary(const Tri &t, int x, int y, double (&l)[3]) {
    const double fx = (double)x, fy = (double)y;
    const double e0 = render_edge(t.u[1], t.v[1], t.u[2], t.v[2], fx, fy);
    const double e1 = render_edge(t.u[2], t.v[2], t.u[0], t.v[0], fx, fy);
    const double e2 = render_edge(t.u[0], t.v[0], t.u[1], t.v[1], fx, fy);
    const bool in = t.A > 0.0 ? (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) : (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
    if (!in) return false;
    l[0] = e0 / t.A; l[1] = e1 / t.A; l[2] = e2 / t.A;
    return true;
}

// The pixel's key, or kRenderEmpty if it is not covered (or its perspective-correct depth is not a finite positive float).
__device__ __forceinline__ unsigned long long render_key(const Tri &t, int x, int y, long f) {
    double l[3];
    if (!render_bary(t, x, y, l)) return kRenderEmpty;
    const double s = l[0] / t.z[0] + l[1] / t.z[1] + l[2] / t.z[2];
    if (!(s > 0.0)) return kRenderEmpty;
    const float zf = (float)(1.0 / s);
    if (!isfinite(zf)) return kRenderEmpty;
    return ((unsigned long long)__float_as_uint(zf) << 32) | (unsigned)f;
}

__device__ __forceinline__ void render_store(unsigned long long *__restrict__ keys, size_t pix, unsigned long long key) {
    if (key < keys[pix]) atomicMin(keys + pix, key);
}

__global__ __launch_bounds__(kRenderBlock) void render_small_kernel(const double *__restrict__ verts, const int *__restrict__ faces,
                                                                    RenderParams p, unsigned long long *__restrict__ keys,
                                                                    unsigned *__restrict__ list_n, unsigned *__restrict__ list) {
    const long i = (long)blockIdx.x * kRenderBlock + threadIdx.x;
    if (i >= (long)p.nv * p.nfaces) return;
    const int view = (int)(i / p.nfaces);
    const long f = i - (long)view * p.nfaces;
    Tri t;
    if (!render_setup(p, p.view[view], verts, faces, f, t)) return;
    const long bw = t.x1 - t.x0 + 1, bh = t.y1 - t.y0 + 1;
    if (bw * bh > kRenderSmallPixels) {
        list[atomicAdd(list_n, 1u)] = (unsigned)i;        // capacity nv * nfaces: never overflows
        return;
    }
    unsigned long long *kv = keys + (size_t)view * p.H * p.W;
    for (int y = t.y0; y <= t.y1; ++y)
        for (int x = t.x0; x <= t.x1; ++x) {
            const unsigned long long key = render_key(t, x, y, f);
            if (key != kRenderEmpty) render_store(kv, (size_t)y * p.W + x, key);
        }
}

__global__ __launch_bounds__(kRenderBlock) void render_large_kernel(const double *__restrict__ verts, const int *__restrict__ faces,
                                                                    RenderParams p, unsigned long long *__restrict__ keys,
                                                                    const unsigned *__restrict__ list_n,
                                                                    const unsigned *__restrict__ list) {
    const unsigned n = *list_n;
    for (unsigned e = blockIdx.x; e < n; e += gridDim.x) {
        const long i = list[e];
        const int view = (int)(i / p.nfaces);
        const long f = i - (long)view * p.nfaces;
        Tri t;
        if (!render_setup(p, p.view[view], verts, faces, f, t)) continue;     // (workgroup-uniform: same inputs for every lane)
        const long bw = t.x1 - t.x0 + 1, npx = bw * (t.y1 - t.y0 + 1);
        unsigned long long *kv = keys + (size_t)view * p.H * p.W;
        for (long q = threadIdx.x; q < npx; q += kRenderBlock) {
            const int y = t.y0 + (int)(q / bw), x = t.x0 + (int)(q - (q / bw) * bw);
            const unsigned long long key = render_key(t, x, y, f);
            if (key != kRenderEmpty) render_store(kv, (size_t)y * p.W + x, key);
        }
    }
}

__global__ __launch_bounds__(kRenderBlock) void render_resolve_kernel(const double *__restrict__ verts, const double *__restrict__ normals,
                                                                      const int *__restrict__ faces, RenderParams p,
                                                                      const unsigned long long *__restrict__ keys, float *__restrict__ depth,
                                                                      int *__restrict__ face_out, float *__restrict__ nrm_out) {
    const long i = (long)blockIdx.x * kRenderBlock + threadIdx.x;
    const long hw = (long)p.H * p.W;
    if (i >= (long)p.nv * hw) return;
    const unsigned long long key = keys[i];
    if (key == kRenderEmpty) {
        depth[i] = 0.0f;
        face_out[i] = -1;
        if (nrm_out) nrm_out[3 * i] = nrm_out[3 * i + 1] = nrm_out[3 * i + 2] = 0.0f;
        return;
    }
    const int f = (int)(unsigned)(key & 0xFFFFFFFFull);
    depth[i] = -__uint_as_float((unsigned)(key >> 32));
    face_out[i] = f;
    if (!nrm_out) return;
    const int view = (int)(i / hw);
    const long pix = i - (long)view * hw;
    const int y = (int)(pix / p.W), x = (int)(pix - (long)y * p.W);
    const RenderView &vw = p.view[view];
    Tri t;
    double l[3];
    double n[3] = {0.0, 0.0, 0.0};
    if (render_setup(p, vw, verts, faces, f, t) && render_bary(t, x, y, l)) {      // (always true: this face wrote the key)
        const double a0 = l[0] / t.z[0], a1 = l[1] / t.z[1], a2 = l[2] / t.z[2];
        const double *n0 = normals + 3 * (size_t)faces[3 * f], *n1 = normals + 3 * (size_t)faces[3 * f + 1],
                     *n2 = normals + 3 * (size_t)faces[3 * f + 2];
        const double m0 = a0 * n0[0] + a1 * n1[0] + a2 * n2[0];
        const double m1 = a0 * n0[1] + a1 * n1[1] + a2 * n2[1];
        const double m2 = a0 * n0[2] + a1 * n1[2] + a2 * n2[2];
        const double *r = vw.r;
        n[0] = r[0] * m0 + r[1] * m1 + r[2] * m2;
        n[1] = r[4] * m0 + r[5] * m1 + r[6] * m2;
        n[2] = r[8] * m0 + r[9] * m1 + r[10] * m2;
        const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (len > 0.0) { n[0] /= len; n[1] /= len; n[2] /= len; }
        else n[0] = n[1] = n[2] = 0.0;
    }
    nrm_out[3 * i] = (float)n[0];
    nrm_out[3 * i + 1] = (float)n[1];
    nrm_out[3 * i + 2] = (float)n[2];
}

struct RenderWorkspace {
    unsigned long long *keys;
    unsigned *list_n, *list;
    size_t bytes;
};

static RenderWorkspace render_workspace(int nv, int H, int W, long nfaces, void *base) {
    RenderWorkspace w;
    size_t off = 0;
    char *b = static_cast<char *>(base);
    auto take = [&](size_t n) { char *r = b ? b + off : nullptr; off += (n + 15) & ~(size_t)15; return r; };
    w.keys = reinterpret_cast<unsigned long long *>(take((size_t)nv * H * W * sizeof(unsigned long long)));
    w.list_n = reinterpret_cast<unsigned *>(take(sizeof(unsigned)));
    w.list = reinterpret_cast<unsigned *>(take((size_t)nv * nfaces * sizeof(unsigned)));
    w.bytes = off;
    return w;
}

static bool render_sizes_ok(int nv, int H, int W, long nfaces) {
    return nv >= 1 && nv <= kRenderMaxViews && H >= 1 && W >= 1 && nfaces >= 0 && nfaces < (1L << 31) &&
           (long)nv * nfaces < (1L << 32) && (long)nv * H * W < (1L << 38);
}

static int render_params(const char *who, int nv, const double *K, const double *lw, int H, int W, long nverts, long nfaces,
                         double scale, const double center[3], double half, double znear, RenderParams &p) {
    DFH_REQUIRE(render_sizes_ok(nv, H, W, nfaces), "%s: bad sizes (views %d in [1, %d], H %d, W %d, faces %ld)", who, nv, kRenderMaxViews,
                H, W, nfaces);
    DFH_REQUIRE(nverts >= 0 && nverts < (1L << 31), "%s: bad vertex count %ld", who, nverts);
    DFH_REQUIRE(K && lw && center, "%s: null host parameter", who);
    DFH_REQUIRE(znear > 0.0, "%s: znear must be > 0", who);
    p.nv = nv; p.H = H; p.W = W; p.nverts = nverts; p.nfaces = nfaces;
    p.scale = scale; p.half = half; p.znear = znear;
    for (int c = 0; c < 3; ++c) p.center[c] = center[c];
    for (int v = 0; v < nv; ++v) {
        const double *k = K + 9 * v;
        DFH_REQUIRE(k[3] == 0.0 && k[6] == 0.0 && k[7] == 0.0 && k[8] == 1.0,
                    "%s: K of view %d must be upper-triangular with last row (0, 0, 1)", who, v);
        p.view[v].k[0] = k[0]; p.view[v].k[1] = k[1]; p.view[v].k[2] = k[2]; p.view[v].k[3] = k[4]; p.view[v].k[4] = k[5];
        for (int j = 0; j < 12; ++j) p.view[v].r[j] = lw[12 * v + j];
    }
    return DFH_OK;
}

// ---- visible-surface samples: the rendered model as the warp solve's sample set (dfh_render_samples_*) ---------------------
// Every `stride`-th pixel of every `stride`-th row (the "lattice", enumerated view-major, then y, then x) whose key is not
// empty yields one sample: attributes of the CANONICAL mesh interpolated perspective-correctly at the pixel with the winning
// face's weights.  Work decomposition (ordered, no atomics -- the pattern of dfh_extract.hip):
//   samples_count_kernel     a workgroup counts the non-empty keys of its kSamplesPix lattice pixels
//   scan_chunks_kernel       (dfh_scan.h) a workgroup scans kSamplesChunk of those counts from zero and leaves the chunk's total
//   scan_chunk_totals_kernel (dfh_scan.h) ONE workgroup scans the chunk totals (64-bit) and stores the count (one plain store)
//   samples_compact_kernel   pass A: the count pass's walk again; every sample learns its rank, the subsample rule picks its
//                            slot, and the kept samples' pixel indices go out -- pixel_out is both a result and pass B's list
//   samples_emit_kernel      pass B: one lane per KEPT sample over that dense list (full waves where a fifth of the image is
//                            covered): key -> face, set-up and weights as in the resolve pass, nine vertex gathers, two rows out
constexpr int kSamplesPix = 1024;     // lattice pixels per workgroup of the count / compact passes (256 lanes x 4)
constexpr int kSamplesChunk = 1024;   // counts per workgroup of the scan (256 lanes x 4): a chunk's total is < 2^20, an int

struct SampleLattice {
    int stride, Hs, Ws, H, W;         // Hs = ceil(H / stride) rows of Ws = ceil(W / stride) lattice pixels per view
    long nl;                          // lattice pixels of all views
};

// pixel index (view * H + y) * W + x of lattice pixel L < nl
__device__ __forceinline__ long lattice_pixel(const SampleLattice &q, long L) {
    if (q.stride == 1) return L;
    long row, view;
    int xs, ys;
    if (q.nl < (1L << 32)) {          // (32-bit divisions where the images allow them)
        const unsigned r = (unsigned)L / (unsigned)q.Ws, v = r / (unsigned)q.Hs;
        xs = (int)((unsigned)L - r * (unsigned)q.Ws);
        ys = (int)(r - v * (unsigned)q.Hs);
        view = v;
    } else {
        row = L / q.Ws;
        xs = (int)(L - row * q.Ws);
        view = row / q.Hs;
        ys = (int)(row - view * q.Hs);
    }
    return (view * q.H + (long)ys * q.stride) * q.W + (long)xs * q.stride;
}

__global__ __launch_bounds__(kRenderBlock) void samples_count_kernel(const unsigned long long *__restrict__ keys, SampleLattice q,
                                                                     int *__restrict__ block_cnt) {
    __shared__ int red[4];
    // lane t takes lattice pixels t, t + 256, t + 512, t + 768 of the workgroup's 1 024: consecutive lanes, consecutive keys
    const long L0 = (long)blockIdx.x * kSamplesPix + threadIdx.x;
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long L = L0 + j * kRenderBlock;
        if (L < q.nl && keys[lattice_pixel(q, L)] != kRenderEmpty) ++c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_cnt[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The scan is dfh_scan.h's two-level pair: block_off[b] = samples of the workgroups of b's chunk in front of b, chunk_tot[chunk] =
// samples of the chunk, chunk_base[c] = samples in front of chunk c, chunk_base[nchunks] = *total_out = all of them
static_assert(kSamplesChunk == 4 * kRenderBlock, "scan_chunks_kernel takes four counts a thread");

__global__ __launch_bounds__(kRenderBlock) void samples_compact_kernel(const unsigned long long *__restrict__ keys, SampleLattice q,
                                                                       const int *__restrict__ block_cnt, const int *__restrict__ block_off,
                                                                       const long *__restrict__ chunk_base, int nchunks, long capacity,
                                                                       long *__restrict__ pixel_out) {
    __shared__ int wave_cnt[4][4];                       // [round j][wave]: samples of lattice pixels j * 256 + 64 * wave .. + 63
    if (block_cnt[blockIdx.x] == 0) return;              // nothing covered here: do not re-read the keys
    const long L0 = (long)blockIdx.x * kSamplesPix + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long pix[4];
    bool ok[4];
    int before[4];                                       // samples of lower lanes of this wave in round j
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long L = L0 + j * kRenderBlock;
        pix[j] = L < q.nl ? lattice_pixel(q, L) : 0;
        ok[j] = L < q.nl && keys[pix[j]] != kRenderEmpty;
        const unsigned long long m = __ballot(ok[j]);
        before[j] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[j][wv] = __popcll(m);
    }
    __syncthreads();
    long at = chunk_base[blockIdx.x / kSamplesChunk] + (long)block_off[blockIdx.x];
    const long total = chunk_base[nchunks];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        long mine = at + before[j];
        for (int w_ = 0; w_ < 4; ++w_) {
            if (w_ < wv) mine += wave_cnt[j][w_];
            at += wave_cnt[j][w_];                       // after the loop: start of round j + 1
        }
        // capacity < total: dfh_surface_emit's EVEN subsample -- sample i goes to slot floor(i * capacity / total) and is kept
        // iff it is the first one of its slot (every slot gets exactly one)
        long dst = mine;
        bool keep = ok[j];
        if (capacity < total) {
            dst = (long)(((__int128)mine * capacity) / total);
            keep = keep && (mine == 0 || (long)(((__int128)(mine - 1) * capacity) / total) != dst);
        }
        if (keep) pixel_out[dst] = pix[j];               // (dst < min(total, capacity): mine < total)
    }
}

__global__ __launch_bounds__(kRenderBlock) void samples_emit_kernel(const double *__restrict__ verts, const double *__restrict__ canon_pos,
                                                                    const double *__restrict__ canon_nrm, const int *__restrict__ faces,
                                                                    RenderParams p, const unsigned long long *__restrict__ keys,
                                                                    const long *__restrict__ chunk_base, int nchunks, long capacity,
                                                                    const long *__restrict__ pixel, double *__restrict__ pos_out,
                                                                    double *__restrict__ nrm_out) {
    const long i = (long)blockIdx.x * kRenderBlock + threadIdx.x;
    const long total = chunk_base[nchunks];
    if (i >= (capacity < total ? capacity : total)) return;
    const long hw = (long)p.H * p.W, pi = pixel[i];
    const long f = (long)(unsigned)(keys[pi] & 0xFFFFFFFFull);
    const int view = (int)(pi / hw);
    const long rem = pi - (long)view * hw;
    const int y = (int)(rem / p.W), x = (int)(rem - (long)y * p.W);
    Tri t;
    double l[3];
    double o[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0};
    // (always true with the raster call's mesh and views: this face wrote the key; another mesh gets zeros, not a wild read)
    if (f < p.nfaces && render_setup(p, p.view[view], verts, faces, f, t) && render_bary(t, x, y, l)) {
        const double a0 = l[0] / t.z[0], a1 = l[1] / t.z[1], a2 = l[2] / t.z[2];
        const double s = (a0 + a1) + a2;
        const double b0 = a0 / s, b1 = a1 / s, b2 = a2 / s;
        const size_t i0 = 3 * (size_t)faces[3 * f], i1 = 3 * (size_t)faces[3 * f + 1], i2 = 3 * (size_t)faces[3 * f + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (b0 * canon_pos[i0 + c] + b1 * canon_pos[i1 + c]) + b2 * canon_pos[i2 + c];
        if (nrm_out) {
            double m[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) m[c] = (b0 * canon_nrm[i0 + c] + b1 * canon_nrm[i1 + c]) + b2 * canon_nrm[i2 + c];
            const double len = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
            if (len > 0.0 && isfinite(len)) { n[0] = m[0] / len; n[1] = m[1] / len; n[2] = m[2] / len; }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) pos_out[3 * i + c] = o[c];
    if (nrm_out) {
#pragma unroll
        for (int c = 0; c < 3; ++c) nrm_out[3 * i + c] = n[c];
    }
}

// ---- K15  vertex ids and the network's input image (dfh_render_vertex_ids) ---------------------------------------------------
// One lane per pixel over the key buffer, like the resolve pass: the winning face's set-up and weights again, the vertex with
// the largest perspective-correct coordinate (the reference's fragment shader rule), and the depth as an 8-bit grey level.
__global__ __launch_bounds__(kRenderBlock) void render_vertex_ids_kernel(const double *__restrict__ verts, const int *__restrict__ faces,
                                                                         RenderParams p, const unsigned long long *__restrict__ keys,
                                                                         double znear_img, double zfar_img, int *__restrict__ vid_out,
                                                                         unsigned char *__restrict__ image_out) {
    const long i = (long)blockIdx.x * kRenderBlock + threadIdx.x;
    const long hw = (long)p.H * p.W;
    if (i >= (long)p.nv * hw) return;
    const unsigned long long key = keys[i];
    int vid = -1;
    int grey = 0;
    if (key != kRenderEmpty) {
        const long f = (long)(unsigned)(key & 0xFFFFFFFFull);
        const float d = __uint_as_float((unsigned)(key >> 32));
        if ((double)d >= znear_img && (double)d <= zfar_img) {
            const float zf = (float)zfar_img, zn = (float)znear_img;
            const float g = ((zf - d) / (zf - zn)) * 255.0f;
            grey = (int)g;                                   // truncation; the float32 images of the two bounds can put g a hair
            grey = grey < 0 ? 0 : (grey > 255 ? 255 : grey); // outside [0, 255]
            const int view = (int)(i / hw);
            const long pix = i - (long)view * hw;
            const int y = (int)(pix / p.W), x = (int)(pix - (long)y * p.W);
            Tri t;
            double l[3];
            // (always true with the raster call's mesh and views: this face wrote the key; another mesh gets -1, not a wild read)
            if (f < p.nfaces && render_setup(p, p.view[view], verts, faces, f, t) && render_bary(t, x, y, l)) {
                const double a0 = l[0] / t.z[0], a1 = l[1] / t.z[1], a2 = l[2] / t.z[2];
                const int w = (a0 > a1 && a0 > a2) ? 0 : (a1 > a2 ? 1 : 2);
                vid = faces[3 * f + w];
            }
        }
    }
    vid_out[i] = vid;
    if (image_out) image_out[i] = (unsigned char)grey;
}

struct SamplesWorkspace {
    int *block_cnt, *block_off;
    long *chunk_tot, *chunk_base;
    long nblocks, nchunks;
    size_t bytes;
};

static bool samples_lattice(int nv, int H, int W, int stride, SampleLattice &q) {
    if (!(nv >= 1 && nv <= kRenderMaxViews && H >= 1 && W >= 1 && stride >= 1 && (long)nv * H * W < (1L << 38))) return false;
    q.stride = stride; q.H = H; q.W = W;
    q.Hs = (H - 1) / stride + 1;
    q.Ws = (W - 1) / stride + 1;
    q.nl = (long)nv * q.Hs * q.Ws;
    return true;
}

static SamplesWorkspace samples_workspace(const SampleLattice &q, void *base) {
    SamplesWorkspace w;
    w.nblocks = (q.nl + kSamplesPix - 1) / kSamplesPix;                  // < 2^28
    w.nchunks = (w.nblocks + kSamplesChunk - 1) / kSamplesChunk;
    size_t off = 0;
    char *b = static_cast<char *>(base);
    auto take = [&](size_t n) { char *r = b ? b + off : nullptr; off += (n + 15) & ~(size_t)15; return r; };
    w.block_cnt = reinterpret_cast<int *>(take((size_t)w.nblocks * sizeof(int)));
    w.block_off = reinterpret_cast<int *>(take((size_t)w.nblocks * sizeof(int)));
    w.chunk_tot = reinterpret_cast<long *>(take((size_t)w.nchunks * sizeof(long)));
    w.chunk_base = reinterpret_cast<long *>(take((size_t)(w.nchunks + 1) * sizeof(long)));
    w.bytes = off;
    return w;
}

}  // namespace dfh

extern "C" {

size_t dfh_render_workspace_bytes(int n_views, int H, int W, long n_faces) {
    using namespace dfh;
    if (!render_sizes_ok(n_views, H, W, n_faces)) return 0;
    return render_workspace(n_views, H, W, n_faces, nullptr).bytes;
}

int dfh_render_raster(const double *verts, long n_verts, const int *faces, long n_faces, int n_views, const double *K, const double *lw,
                      int H, int W, double scale, const double center[3], double half, double znear, void *workspace,
                      size_t workspace_bytes, void *stream) {
    using namespace dfh;
    RenderParams p;
    const int rc = render_params("dfh_render_raster", n_views, K, lw, H, W, n_verts, n_faces, scale, center, half, znear, p);
    if (rc != DFH_OK) return rc;
    DFH_REQUIRE(workspace, "dfh_render_raster: null workspace");
    DFH_REQUIRE(workspace_bytes >= dfh_render_workspace_bytes(n_views, H, W, n_faces), "dfh_render_raster: workspace too small");
    DFH_REQUIRE(n_faces == 0 || (faces && verts), "dfh_render_raster: null mesh");
    const RenderWorkspace w = render_workspace(n_views, H, W, n_faces, workspace);
    hipStream_t s = (hipStream_t)stream;
    DFH_HIP_CHECK(hipMemsetAsync(w.keys, 0xFF, (size_t)n_views * H * W * sizeof(unsigned long long), s));
    DFH_HIP_CHECK(hipMemsetAsync(w.list_n, 0, sizeof(unsigned), s));
    const long npairs = (long)n_views * n_faces;
    if (npairs == 0) return DFH_OK;
    const long nb = (npairs + kRenderBlock - 1) / kRenderBlock;
    DFH_REQUIRE(nb < (1L << 31), "dfh_render_raster: too many triangles");
    hipLaunchKernelGGL(render_small_kernel, dim3((unsigned)nb), dim3(kRenderBlock), 0, s, verts, faces, p, w.keys, w.list_n, w.list);
    int dev = 0;
    DFH_HIP_CHECK(hipGetDevice(&dev));
    DeviceInfo &di = device_info(dev);
    if (di.n_cu == 0) DFH_HIP_CHECK(hipDeviceGetAttribute(&di.n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    const long ng = nb < 4L * di.n_cu ? nb : 4L * di.n_cu;    // the large pairs' count stays on the device: a fixed grid pulls them
    hipLaunchKernelGGL(render_large_kernel, dim3((unsigned)ng), dim3(kRenderBlock), 0, s, verts, faces, p, w.keys, w.list_n, w.list);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_render_resolve(const double *verts, const double *normals, long n_verts, const int *faces, long n_faces, int n_views,
                       const double *K, const double *lw, int H, int W, double scale, const double center[3], double half, double znear,
                       const void *workspace, size_t workspace_bytes, float *depth_out, int *face_out, float *normal_out, void *stream) {
    using namespace dfh;
    RenderParams p;
    const int rc = render_params("dfh_render_resolve", n_views, K, lw, H, W, n_verts, n_faces, scale, center, half, znear, p);
    if (rc != DFH_OK) return rc;
    DFH_REQUIRE(workspace, "dfh_render_resolve: null workspace");
    DFH_REQUIRE(workspace_bytes >= dfh_render_workspace_bytes(n_views, H, W, n_faces), "dfh_render_resolve: workspace too small");
    DFH_REQUIRE(depth_out && face_out, "dfh_render_resolve: null output");
    DFH_REQUIRE((normals == nullptr) == (normal_out == nullptr), "dfh_render_resolve: normals and normal_out go together");
    DFH_REQUIRE(n_faces == 0 || (faces && verts), "dfh_render_resolve: null mesh");
    const RenderWorkspace w = render_workspace(n_views, H, W, n_faces, const_cast<void *>(workspace));
    const long npix = (long)n_views * H * W;
    hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((npix + kRenderBlock - 1) / kRenderBlock)), dim3(kRenderBlock), 0,
                       (hipStream_t)stream, verts, normals, faces, p, w.keys, depth_out, face_out, normal_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

size_t dfh_render_samples_workspace_bytes(int n_views, int H, int W, int stride) {
    using namespace dfh;
    SampleLattice q;
    if (!samples_lattice(n_views, H, W, stride, q)) return 0;
    return samples_workspace(q, nullptr).bytes;
}

int dfh_render_samples_count(int n_views, int H, int W, long n_faces, int stride, const void *workspace, size_t workspace_bytes,
                             void *scan_workspace, size_t scan_workspace_bytes, long *total_out, void *stream) {
    using namespace dfh;
    SampleLattice q;
    DFH_REQUIRE(render_sizes_ok(n_views, H, W, n_faces), "dfh_render_samples_count: bad sizes (views %d in [1, %d], H %d, W %d, faces %ld)",
                n_views, kRenderMaxViews, H, W, n_faces);
    DFH_REQUIRE(stride >= 1 && samples_lattice(n_views, H, W, stride, q), "dfh_render_samples_count: stride %d must be >= 1", stride);
    DFH_REQUIRE(workspace && scan_workspace && total_out, "dfh_render_samples_count: null pointer");
    DFH_REQUIRE(workspace_bytes >= dfh_render_workspace_bytes(n_views, H, W, n_faces), "dfh_render_samples_count: workspace too small");
    DFH_REQUIRE(scan_workspace_bytes >= dfh_render_samples_workspace_bytes(n_views, H, W, stride),
                "dfh_render_samples_count: scan workspace too small");
    const RenderWorkspace w = render_workspace(n_views, H, W, n_faces, const_cast<void *>(workspace));
    const SamplesWorkspace sw = samples_workspace(q, scan_workspace);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(samples_count_kernel, dim3((unsigned)sw.nblocks), dim3(kRenderBlock), 0, s, w.keys, q, sw.block_cnt);
    hipLaunchKernelGGL((scan_chunks_kernel<int, long, kRenderBlock / kWave>), dim3((unsigned)sw.nchunks), dim3(kRenderBlock), 0, s,
                       (const int *)sw.block_cnt, (long)sw.nblocks, sw.block_off, sw.chunk_tot);
    hipLaunchKernelGGL((scan_chunk_totals_kernel<long, kRenderBlock / kWave>), dim3(1), dim3(kRenderBlock), 0, s, (const long *)sw.chunk_tot,
                       (long)sw.nchunks, sw.chunk_base, total_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_render_samples_emit(const double *verts, const double *canon_pos, const double *canon_nrm, long n_verts, const int *faces,
                            long n_faces, int n_views, const double *K, const double *lw, int H, int W, double scale, const double center[3],
                            double half, double znear, int stride, const void *workspace, size_t workspace_bytes,
                            const void *scan_workspace, size_t scan_workspace_bytes, double *pos_out, double *nrm_out, long *pixel_out,
                            long capacity, void *stream) {
    using namespace dfh;
    RenderParams p;
    SampleLattice q;
    const int rc = render_params("dfh_render_samples_emit", n_views, K, lw, H, W, n_verts, n_faces, scale, center, half, znear, p);
    if (rc != DFH_OK) return rc;
    DFH_REQUIRE(stride >= 1 && samples_lattice(n_views, H, W, stride, q), "dfh_render_samples_emit: stride %d must be >= 1", stride);
    DFH_REQUIRE(capacity >= 0, "dfh_render_samples_emit: capacity %ld < 0", capacity);
    DFH_REQUIRE(workspace && scan_workspace, "dfh_render_samples_emit: null workspace");
    DFH_REQUIRE(workspace_bytes >= dfh_render_workspace_bytes(n_views, H, W, n_faces), "dfh_render_samples_emit: workspace too small");
    DFH_REQUIRE(scan_workspace_bytes >= dfh_render_samples_workspace_bytes(n_views, H, W, stride),
                "dfh_render_samples_emit: scan workspace too small");
    DFH_REQUIRE(n_faces == 0 || (faces && verts && canon_pos), "dfh_render_samples_emit: null mesh");
    DFH_REQUIRE(canon_nrm || !nrm_out, "dfh_render_samples_emit: a normal output needs canon_nrm");
    if (capacity == 0 || n_faces == 0) return DFH_OK;                 // (no faces: nothing is covered, no row is written)
    DFH_REQUIRE(pos_out && pixel_out, "dfh_render_samples_emit: null output");
    const RenderWorkspace w = render_workspace(n_views, H, W, n_faces, const_cast<void *>(workspace));
    const SamplesWorkspace sw = samples_workspace(q, const_cast<void *>(scan_workspace));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(samples_compact_kernel, dim3((unsigned)sw.nblocks), dim3(kRenderBlock), 0, s, (const unsigned long long *)w.keys, q,
                       (const int *)sw.block_cnt, (const int *)sw.block_off, (const long *)sw.chunk_base, (int)sw.nchunks, capacity, pixel_out);
    const long rows = capacity < q.nl ? capacity : q.nl;               // (the count stays on the device: lanes beyond it return)
    hipLaunchKernelGGL(samples_emit_kernel, dim3((unsigned)((rows + kRenderBlock - 1) / kRenderBlock)), dim3(kRenderBlock), 0, s, verts,
                       canon_pos, canon_nrm, faces, p, (const unsigned long long *)w.keys, (const long *)sw.chunk_base, (int)sw.nchunks,
                       capacity, (const long *)pixel_out, pos_out, nrm_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_render_vertex_ids(const double *verts, long n_verts, const int *faces, long n_faces, int n_views, const double *K, const double *lw,
                          int H, int W, double scale, const double center[3], double half, double znear, const void *workspace,
                          size_t workspace_bytes, double znear_img, double zfar_img, int *vid_out, unsigned char *image_out, void *stream) {
    using namespace dfh;
    RenderParams p;
    const int rc = render_params("dfh_render_vertex_ids", n_views, K, lw, H, W, n_verts, n_faces, scale, center, half, znear, p);
    if (rc != DFH_OK) return rc;
    DFH_REQUIRE(std::isfinite(znear_img) && std::isfinite(zfar_img) && zfar_img > znear_img,
                "dfh_render_vertex_ids: the image range needs finite znear_img < zfar_img");
    DFH_REQUIRE(workspace, "dfh_render_vertex_ids: null workspace");
    DFH_REQUIRE(workspace_bytes >= dfh_render_workspace_bytes(n_views, H, W, n_faces), "dfh_render_vertex_ids: workspace too small");
    DFH_REQUIRE(vid_out, "dfh_render_vertex_ids: null output");
    DFH_REQUIRE(n_faces == 0 || (faces && verts), "dfh_render_vertex_ids: null mesh");
    const RenderWorkspace w = render_workspace(n_views, H, W, n_faces, const_cast<void *>(workspace));
    const long npix = (long)n_views * H * W;
    hipLaunchKernelGGL(render_vertex_ids_kernel, dim3((unsigned)((npix + kRenderBlock - 1) / kRenderBlock)), dim3(kRenderBlock), 0,
                       (hipStream_t)stream, verts, faces, p, (const unsigned long long *)w.keys, znear_img, zfar_img, vid_out, image_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

}  // extern "C"
