/* oracle_c.c -- plain C restatement of the reference's hot path (CPU semantics): A1 depth -> TSDF integration, A3 rigid and A4
 * non-rigid (DQB) TSDF -> TSDF fusion.
 * TEST INFRASTRUCTURE ONLY: loaded by tests/ and by bench.py's cpu_baseline leg through ctypes
 * (oracle/oracle_c.py); never by the product.
 *
 * Restates FusionDM.fuseDepths (reference core/fusion_dm.py:180-217), FusionDM.updateTSDF (:300-316) and Fusion.updateTSDF
 * (core/fusion.py:153-198) one voxel at a time in the operation order of oracle/oracle_np.py, which follows the reference's
 * (compile with -ffp-contract=off: no fused multiply-add), float64 volumes, float64 or float32 depth / live volume.
 * Pinned: tests/test_oracle_c.py checks it against the numpy oracle and against the vectors produced by running the reference
 * (tests/golden/g2, g3, g4, g6): A1 and A3 bit for bit, A4 to 1e-12 (libm exp() against numpy's).
 * OpenMP over the slowest axis: voxels are independent (np.nditer order is irrelevant to the result).
 */
#include <math.h>
#include <stddef.h>

#ifdef _OPENMP
#include <omp.h>
#endif

int oracle_c_threads(void) {
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}

/* returns the number of updated voxels; tsdf / tsdf_w: X*Y*Z doubles, C order (z fastest) */
long oracle_c_fuse_depths(double *tsdf, double *tsdf_w, int X, int Y, int Z, int tsdf_res, int x0, int x1,
                          const void *depth, int depth_is_f32, int H, int W, const double *K, const double *Kinv,
                          const double *lw, double scale, const double *center, double tdist, double wmax,
                          int n_threads) {
    const double c = (double)tsdf_res / 2.0;                 /* sdf_center, :183 */
    const float *d32 = (const float *)depth;
    const double *d64 = (const double *)depth;
    long count = 0;
#ifdef _OPENMP
    if (n_threads > 0) omp_set_num_threads(n_threads);
#pragma omp parallel for schedule(static) reduction(+ : count)
#endif
    for (int x = x0; x < x1; ++x) {
        for (int y = 0; y < Y; ++y) {
            for (int z = 0; z < Z; ++z) {
                /* pos = scale*(i - c) + center                         (:188-191) */
                const double px = scale * ((double)(float)x - c) + center[0];
                const double py = scale * ((double)(float)y - c) + center[1];
                const double pz = scale * ((double)(float)z - c) + center[2];
                /* lpos = lw @ [pos,1]                                   (:193) */
                const double l0 = ((lw[0] * px + lw[1] * py) + lw[2] * pz) + lw[3];
                const double l1 = ((lw[4] * px + lw[5] * py) + lw[6] * pz) + lw[7];
                const double l2 = ((lw[8] * px + lw[9] * py) + lw[10] * pz) + lw[11];
                /* project_to_pixel(K, lpos)                             (:194, util.py:317-320) */
                const double p0 = (K[0] * l0 + K[1] * l1) + K[2] * l2;
                const double p1 = (K[3] * l0 + K[4] * l1) + K[5] * l2;
                const double p2 = (K[6] * l0 + K[7] * l1) + K[8] * l2;
                if (!(p2 != 0.0)) continue;
                const double u = p0 / p2, v = p1 / p2;
                if (!(u >= 0.0 && u < (double)(W - 1) && v >= 0.0 && v < (double)(H - 1))) continue;   /* :195 */
                const long ui = lrint(u), vi = lrint(v);         /* round half to even (:196) */
                const double dz = depth_is_f32 ? (double)d32[vi * W + ui] : d64[vi * W + ui];
                const double zd = -1.0 * dz;
                if (!(zd > 0.0)) continue;                       /* :197 */
                const double cz = (Kinv[6] * (zd * u) + Kinv[7] * (zd * v)) + Kinv[8] * (zd * 1.0);  /* :198-200 */
                const double sd = cz - l2;                       /* :201 */
                if (!(sd > -1.0 * tdist)) continue;              /* :203 */
                const size_t i = ((size_t)x * Y + y) * Z + z;
                const double wt = tsdf_w[i];
                const double m = sd < tdist ? sd : tdist;
                tsdf[i] = (scale * tsdf[i] * wt + m * 1.0) / (scale * (1.0 + wt));     /* :209 */
                const double nw = 1.0 + wt;
                tsdf_w[i] = nw < wmax ? nw : wmax;               /* :210 */
                ++count;
            }
        }
    }
    return count;
}

/* ------------------------------------------------------------------------------------------------------------------------------
 * A3 / A4: TSDF -> TSDF fusion.  Restates oracle_np.update_tsdf_rigid (FusionDM.updateTSDF, reference core/fusion_dm.py:300-316)
 * and oracle_np.update_tsdf_dqb (Fusion.updateTSDF, core/fusion.py:153-198) voxel by voxel in numpy's operation order.  The live
 * volume (float32 or float64, extent LX x LY x LZ, any size) is read in place; its values widen to double exactly.
 * Two forms each: (a) in place on float64 T / w volumes that hold planes [xb, xb + nxT) of the grid, sweeping planes [x0, x1);
 * (b) a list of flat voxel indices ((x * Y + y) * Z + z) with per-voxel T / w in and T / w / update flag out.
 * Pinned: tests/test_oracle_c.py (bit for bit against oracle_np for A3; A4 to 1e-12: libm exp() against numpy's, and golden
 * g3 / g4, the reference's own outputs).
 * ------------------------------------------------------------------------------------------------------------------------------ */
#define ORACLE_KMAX 8

typedef struct {
    const void *p;
    int f32, LX, LY, LZ;
} live_t;

static inline double live_at(const live_t *L, long x, long y, long z) {
    const size_t i = ((size_t)x * L->LY + y) * L->LZ + z;
    return L->f32 ? (double)((const float *)L->p)[i] : ((const double *)L->p)[i];
}

/* oracle_np.quaternion_multiply (core/util.py:255-269), w-first, left to right as numpy evaluates the expressions */
static void qmul(const double *q1, const double *q0, double *o) {
    const double w0 = q0[0], x0 = q0[1], y0 = q0[2], z0 = q0[3];
    const double w1 = q1[0], x1 = q1[1], y1 = q1[2], z1 = q1[3];
    o[0] = ((-x1 * x0 - y1 * y0) - z1 * z0) + w1 * w0;
    o[1] = ((x1 * w0 + y1 * z0) - z1 * y0) + w1 * x0;
    o[2] = ((-x1 * z0 + y1 * w0) + z1 * x0) + w1 * y0;
    o[3] = ((x1 * y0 - y1 * x0) + z1 * w0) + w1 * z0;
}

/* dual_quaternion_multiply (core/util.py:275-282) */
static void dqmul(const double *a, const double *b, double *o) {
    double t0[4], t1[4];
    qmul(a, b, o);
    qmul(a, b + 4, t0);
    qmul(a + 4, b, t1);
    for (int i = 0; i < 4; ++i) o[4 + i] = t0[i] + t1[i];
}

/* dqb_warp (core/util.py:68-72): the point is rounded to float32 first (vq dtype) */
static void dqb_warp(const double *dq, const double *pos, double *out) {
    const double vq[8] = {1.0, 0.0, 0.0, 0.0, 0.0, (double)(float)pos[0], (double)(float)pos[1], (double)(float)pos[2]};
    const double cj[8] = {dq[0], -dq[1], -dq[2], -dq[3], -dq[4], dq[5], dq[6], dq[7]};
    double dqv[8], r[8];
    dqmul(dq, vq, dqv);
    dqmul(dqv, cj, r);
    out[0] = r[5]; out[1] = r[6]; out[2] = r[7];
}

/* interpolate_tsdf (core/util.py:102-137): ceil() corners, the y-fraction blends the z1 samples and the z-fraction the y1
 * samples.  Returns 0 where the reference returns None (outside, or not finite). */
static int interp(const live_t *L, const double *q, double *val) {
    const double px = q[0], py = q[1], pz = q[2];
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) return 0;
    const double mn = fmin(fmin(px, py), pz);
    if (mn < 0.0 || px > (double)(L->LX - 1) || py > (double)(L->LY - 1) || pz > (double)(L->LZ - 1)) return 0;
    const long x0 = (long)floor(px), x1 = (long)ceil(px);
    const long y0 = (long)floor(py), y1 = (long)ceil(py);
    const long z0 = (long)floor(pz), z1 = (long)ceil(pz);
    const double xd = px - (double)x0, yd = py - (double)y0, zd = pz - (double)z0;
    const double c000 = live_at(L, x0, y0, z0), c100 = live_at(L, x1, y0, z0);
    const double c001 = live_at(L, x0, y1, z0), c101 = live_at(L, x1, y1, z0);
    const double c010 = live_at(L, x0, y0, z1), c110 = live_at(L, x1, y0, z1);
    const double c011 = live_at(L, x0, y1, z1), c111 = live_at(L, x1, y1, z1);
    const double c00 = c000 * (1.0 - xd) + c100 * xd;
    const double c01 = c001 * (1.0 - xd) + c101 * xd;
    const double c10 = c010 * (1.0 - xd) + c110 * xd;
    const double c11 = c011 * (1.0 - xd) + c111 * xd;
    const double c0 = c00 * (1.0 - yd) + c10 * yd;
    const double c1 = c01 * (1.0 - yd) + c11 * yd;
    *val = c0 * (1.0 - zd) + c1 * zd;
    return 1;
}

/* the float32 multi_index of np.nditer (fusion_dm.py:186-188, fusion.py:169-171) */
static inline void voxel_pos(long x, long y, long z, double *pos) {
    pos[0] = (double)(float)x; pos[1] = (double)(float)y; pos[2] = (double)(float)z;
}

/* one voxel of A3 (fusion_dm.py:306-312); returns the update flag */
static int rigid_voxel(const live_t *L, const double *lw, double tdist, double wmax, long x, long y, long z,
                       double T, double W, double *To, double *Wo) {
    double pos[3], q[3], s;
    voxel_pos(x, y, z, pos);
    dqb_warp(lw, pos, q);                                                       /* :306 */
    if (!interp(L, q, &s) || !(s > -1.0 * tdist)) { *To = T; *Wo = W; return 0; }   /* :307-308 */
    const double m = s < tdist ? s : tdist;
    *To = (T * W + m * 1.0) / (1.0 + W);                                       /* :309-312 via _avg_update(wi = 1) */
    const double nw = 1.0 + W;
    *Wo = nw < wmax ? nw : wmax;
    return 1;
}

typedef struct {
    const double *pos, *dq, *w;
    int N, k;
} nodes_t;

/* one voxel of A4 (fusion.py:169-190) */
static int dqb_voxel(const live_t *L, const nodes_t *G, const double *lw, double tdist, double wmax, long x, long y, long z,
                     double T, double W, double *To, double *Wo) {
    const int k = G->k;
    double pos[3];
    voxel_pos(x, y, z, pos);
    /* knn_bruteforce: ascending squared distance, ties to the lower node index (stable argsort)        (:175-176) */
    double bd[ORACLE_KMAX];
    int bi[ORACLE_KMAX];
    for (int j = 0; j < k; ++j) { bd[j] = INFINITY; bi[j] = -1; }
    for (int n = 0; n < G->N; ++n) {
        const double dx = pos[0] - G->pos[3 * n], dy = pos[1] - G->pos[3 * n + 1], dz = pos[2] - G->pos[3 * n + 2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (!(d2 < bd[k - 1]) && bi[k - 1] >= 0) continue;
        int j = k - 1;
        while (j > 0 && (bi[j - 1] < 0 || d2 < bd[j - 1])) { bd[j] = bd[j - 1]; bi[j] = bi[j - 1]; --j; }
        bd[j] = d2; bi[j] = n;
    }
    /* dq_blend (:527-551): Gaussian weights, sigma = 2 * node_w; normalised by the full 8-norm; zero blend -> identity */
    double b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < k; ++j) {
        const double *np_ = G->pos + 3 * bi[j];
        const double ex = pos[0] - np_[0], ey = pos[1] - np_[1], ez = pos[2] - np_[2];
        const double dist = sqrt((ex * ex + ey * ey) + ez * ez);
        const double t = dist / (2.0 * G->w[bi[j]]);
        const double wj = exp(-1.0 * (t * t));
        for (int c = 0; c < 8; ++c) b[c] = b[c] + wj * G->dq[8 * bi[j] + c];
    }
    double sq[8];
    for (int c = 0; c < 8; ++c) sq[c] = b[c] * b[c];
    const double n8 = sqrt(((sq[0] + sq[1]) + (sq[2] + sq[3])) + ((sq[4] + sq[5]) + (sq[6] + sq[7])));   /* np.sum, pairwise */
    double se3[8];
    if (n8 == 0.0) {
        for (int c = 0; c < 8; ++c) se3[c] = c == 0 ? 1.0 : 0.0;
    } else {
        for (int c = 0; c < 8; ++c) se3[c] = b[c] / n8;
    }
    double pw[3], q[3], s;
    dqb_warp(se3, pos, pw);                                                     /* warp, :510 */
    dqb_warp(lw, pw, q);                                                        /* m_lw, :512 (re-rounds to float32) */
    if (!interp(L, q, &s) || !(s > -1.0 * tdist)) { *To = T; *Wo = W; return 0; }   /* :179 */
    double wi = 0.0;                                                            /* :182-183 */
    for (int j = 0; j < k; ++j) {
        const double *np_ = G->pos + 3 * bi[j];
        const double ex = np_[0] - pos[0], ey = np_[1] - pos[1], ez = np_[2] - pos[2];
        wi = wi + sqrt((ex * ex + ey * ey) + ez * ez) / (double)k;
    }
    const double Wt = W == 0.0 ? wi : W;                                        /* :186-187 */
    const double m = s < tdist ? s : tdist;
    *To = (T * Wt + m * wi) / (wi + Wt);                                        /* :189-190 */
    const double nw = wi + Wt;
    *Wo = nw < wmax ? nw : wmax;
    return 1;
}

/* form (a) of both: returns the number of updated voxels; mask (nullable) is a byte per voxel of T's layout */
static long tsdf_update_volume(int dqb, double *tsdf, double *tsdf_w, unsigned char *mask, int xb, int nxT, int Y, int Z, int x0,
                               int x1, const live_t *L, const nodes_t *G, const double *lw, double tdist, double wmax, int n_threads) {
    long count = 0;
    if (x0 < xb) x0 = xb;
    if (x1 > xb + nxT) x1 = xb + nxT;
#ifdef _OPENMP
    if (n_threads > 0) omp_set_num_threads(n_threads);
#pragma omp parallel for collapse(2) schedule(dynamic, 1) reduction(+ : count)
#endif
    for (int x = x0; x < x1; ++x) {
        for (int y = 0; y < Y; ++y) {
            for (int z = 0; z < Z; ++z) {
                const size_t i = ((size_t)(x - xb) * Y + y) * Z + z;
                double To, Wo;
                const int u = dqb ? dqb_voxel(L, G, lw, tdist, wmax, x, y, z, tsdf[i], tsdf_w[i], &To, &Wo)
                                  : rigid_voxel(L, lw, tdist, wmax, x, y, z, tsdf[i], tsdf_w[i], &To, &Wo);
                tsdf[i] = To; tsdf_w[i] = Wo;
                if (mask) mask[i] = (unsigned char)u;
                count += u;
            }
        }
    }
    return count;
}

/* form (b) of both */
static long tsdf_update_list(int dqb, const long long *idx, long n, int X, int Y, int Z, const double *T_in, const double *W_in,
                             double *T_out, double *W_out, unsigned char *mask, const live_t *L, const nodes_t *G, const double *lw,
                             double tdist, double wmax, int n_threads) {
    long count = 0, bad = 0;
#ifdef _OPENMP
    if (n_threads > 0) omp_set_num_threads(n_threads);
#pragma omp parallel for schedule(dynamic, 256) reduction(+ : count, bad)
#endif
    for (long j = 0; j < n; ++j) {
        const long long f = idx[j];
        if (f < 0 || f >= (long long)X * Y * Z) { ++bad; continue; }
        const long z = (long)(f % Z), y = (long)((f / Z) % Y), x = (long)(f / ((long long)Y * Z));
        double To, Wo;
        const int u = dqb ? dqb_voxel(L, G, lw, tdist, wmax, x, y, z, T_in[j], W_in[j], &To, &Wo)
                          : rigid_voxel(L, lw, tdist, wmax, x, y, z, T_in[j], W_in[j], &To, &Wo);
        T_out[j] = To; W_out[j] = Wo;
        mask[j] = (unsigned char)u;
        count += u;
    }
    return bad ? -1 : count;
}

long oracle_c_update_tsdf_rigid(double *tsdf, double *tsdf_w, unsigned char *mask, int xb, int nxT, int Y, int Z, int x0, int x1,
                                const void *live, int live_is_f32, const int live_res[3], const double *lw_dq, double tdist,
                                double wmax, int n_threads) {
    const live_t L = {live, live_is_f32, live_res[0], live_res[1], live_res[2]};
    return tsdf_update_volume(0, tsdf, tsdf_w, mask, xb, nxT, Y, Z, x0, x1, &L, NULL, lw_dq, tdist, wmax, n_threads);
}

long oracle_c_update_tsdf_rigid_list(const long long *idx, long n, const int res[3], const double *T_in, const double *W_in,
                                     double *T_out, double *W_out, unsigned char *mask, const void *live, int live_is_f32,
                                     const int live_res[3], const double *lw_dq, double tdist, double wmax, int n_threads) {
    const live_t L = {live, live_is_f32, live_res[0], live_res[1], live_res[2]};
    return tsdf_update_list(0, idx, n, res[0], res[1], res[2], T_in, W_in, T_out, W_out, mask, &L, NULL, lw_dq, tdist, wmax,
                            n_threads);
}

long oracle_c_update_tsdf_dqb(double *tsdf, double *tsdf_w, unsigned char *mask, int xb, int nxT, int Y, int Z, int x0, int x1,
                              const void *live, int live_is_f32, const int live_res[3], const double *node_pos,
                              const double *node_dq, const double *node_w, int n_nodes, int knn, const double *lw_dq,
                              double tdist, double wmax, int n_threads) {
    if (knn < 1 || knn > ORACLE_KMAX || n_nodes < knn) return -1;
    const live_t L = {live, live_is_f32, live_res[0], live_res[1], live_res[2]};
    const nodes_t G = {node_pos, node_dq, node_w, n_nodes, knn};
    return tsdf_update_volume(1, tsdf, tsdf_w, mask, xb, nxT, Y, Z, x0, x1, &L, &G, lw_dq, tdist, wmax, n_threads);
}

long oracle_c_update_tsdf_dqb_list(const long long *idx, long n, const int res[3], const double *T_in, const double *W_in,
                                   double *T_out, double *W_out, unsigned char *mask, const void *live, int live_is_f32,
                                   const int live_res[3], const double *node_pos, const double *node_dq, const double *node_w,
                                   int n_nodes, int knn, const double *lw_dq, double tdist, double wmax, int n_threads) {
    if (knn < 1 || knn > ORACLE_KMAX || n_nodes < knn) return -1;
    const live_t L = {live, live_is_f32, live_res[0], live_res[1], live_res[2]};
    const nodes_t G = {node_pos, node_dq, node_w, n_nodes, knn};
    return tsdf_update_list(1, idx, n, res[0], res[1], res[2], T_in, W_in, T_out, W_out, mask, &L, &G, lw_dq, tdist, wmax,
                            n_threads);
}
