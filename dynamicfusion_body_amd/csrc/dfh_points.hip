// Point-cloud and deformation-graph queries, and the residual evaluators with the reference's definitions, for parity:
//      dfh_residual_rigid  = FusionDM.computef_lw      (reference core/fusion_dm.py:285-297)
//      dfh_residual_data   = data rows of Fusion.computef / computef_lw (core/fusion.py:444-473)
//      dfh_residual_reg    = regularisation rows of Fusion.computef     (core/fusion.py:475-484)
// with the rigid 6-DoF normal equations of the global `_lw`, the batch warp (Fusion.warp, core/fusion.py:502-520), the
// selection loop of setupCorrespondences (core/fusion_dm.py:229-244), the device side of update_graph / construct_graph
// (core/fusion.py:101-123, 201-239) and the per-sample node search with its static blend weights.
//
// Everything is fp64 with the reference's operation order: the evaluators are bit-comparable with the CPU path.
#include "dfh_solve_math.h"

namespace dfh {

// ------------------------------------------------------------------------------- residuals
__global__ __launch_bounds__(256) void residual_rigid_kernel(const double *__restrict__ verts, const double *__restrict__ norms,
                                                              const double *__restrict__ corr, int n, DQ x,
                                                              double *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const D3 wn = dqb_warp_normal_exact(x.q, round_f32(norms[3 * i]), round_f32(norms[3 * i + 1]), round_f32(norms[3 * i + 2]));
    const D3 vp = dqb_warp_exact(x.q, round_f32(verts[3 * i]), round_f32(verts[3 * i + 1]), round_f32(verts[3 * i + 2]));
    const double d0 = vp.x - corr[3 * i], d1 = vp.y - corr[3 * i + 1], d2 = vp.z - corr[3 * i + 2];
    out[i] = (wn.x * d0 + wn.y * d1) + wn.z * d2;                    // fusion_dm.py:293
}

__global__ __launch_bounds__(256) void residual_data_kernel(const double *__restrict__ verts, const double *__restrict__ norms,
                                                             const double *__restrict__ corr, const int *__restrict__ nbr,
                                                             int V, int k, const double *__restrict__ node_dq,
                                                             const double *__restrict__ node_pos,
                                                             const double *__restrict__ node_w, DQ lw,
                                                             double *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    int idx[kKMaxS];
#pragma unroll
    for (int j = 0; j < kKMaxS; ++j) idx[j] = j < k ? nbr[(size_t)i * k + j] : 0;
    const double px = verts[3 * i], py = verts[3 * i + 1], pz = verts[3 * i + 2];
    double bh[8];
    blend_from_indices(node_dq, node_pos, node_w, idx, k, px, py, pz, bh, nullptr, nullptr);     // fusion.py:508
    const D3 x1 = dqb_warp_exact(bh, round_f32(px), round_f32(py), round_f32(pz));                // :510
    const D3 xp = dqb_warp_exact(lw.q, round_f32(x1.x), round_f32(x1.y), round_f32(x1.z));        // :512
    const D3 n1 = dqb_warp_normal_exact(bh, round_f32(norms[3 * i]), round_f32(norms[3 * i + 1]), round_f32(norms[3 * i + 2]));  // :515
    const D3 np_ = dqb_warp_normal_exact(lw.q, round_f32(n1.x), round_f32(n1.y), round_f32(n1.z));                             // :517
    const double d0 = xp.x - corr[3 * i], d1 = xp.y - corr[3 * i + 1], d2 = xp.z - corr[3 * i + 2];
    out[i] = (np_.x * d0 + np_.y * d1) + np_.z * d2;                 // fusion.py:470
}

__global__ __launch_bounds__(256) void residual_reg_kernel(const int *__restrict__ node_nbr, int N, int k,
                                                            const double *__restrict__ node_dq,
                                                            const double *__restrict__ node_pos,
                                                            const double *__restrict__ node_w, double rw,
                                                            double *__restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= N * k) return;
    const int i = t / k;
    const int j = node_nbr[t];
    const double vx = round_f32(node_pos[3 * j]), vy = round_f32(node_pos[3 * j + 1]), vz = round_f32(node_pos[3 * j + 2]);
    const D3 yi = dqb_warp_exact(node_dq + 8 * i, vx, vy, vz);
    const D3 yj = dqb_warp_exact(node_dq + 8 * j, vx, vy, vz);
    const double wi = node_w[i], wj = node_w[j];
    const double c = rw * (wi > wj ? wi : wj);                       // rw * max(w_i, w_j), fusion.py:482
    out[3 * t + 0] = c * (yi.x - yj.x);
    out[3 * t + 1] = c * (yi.y - yj.y);
    out[3 * t + 2] = c * (yi.z - yj.z);
}

// Rigid 6-DoF normal equations for the global `_lw`: r_i as above, J_i = [ c_i x m_i | s m_i ]
// (m = warped normal, s = |r_x|^2; derivation in oracle/gn_np.py).  out: 36 (J^T J) + 6 (J^T r)
// + 1 (0.5|r|^2) + 1 (count) doubles.  partial != NULL: every workgroup stores its 29 sums (row blockIdx.x of `partial`) and
// gn_rigid_finish_kernel adds the rows in a fixed order -- same bits every run; partial == NULL (no scratch to be had): one
// atomic per workgroup and entry into `out`.
__global__ __launch_bounds__(256) void gn_build_rigid_kernel(const double *__restrict__ verts, const double *__restrict__ norms,
                                                              const double *__restrict__ corr,
                                                              const unsigned char *__restrict__ valid, int n, DQ x,
                                                              double *__restrict__ out, double *__restrict__ partial) {
    __shared__ double red[256];
    double acc[29];
    for (int e = 0; e < 29; ++e) acc[e] = 0.0;
    const double s = (x.q[0] * x.q[0] + x.q[1] * x.q[1]) + (x.q[2] * x.q[2] + x.q[3] * x.q[3]);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (valid && !valid[i]) continue;
        const D3 m = dqb_warp_normal_exact(x.q, round_f32(norms[3 * i]), round_f32(norms[3 * i + 1]), round_f32(norms[3 * i + 2]));
        const D3 y = dqb_warp_exact(x.q, round_f32(verts[3 * i]), round_f32(verts[3 * i + 1]), round_f32(verts[3 * i + 2]));
        const double c0 = corr[3 * i], c1 = corr[3 * i + 1], c2 = corr[3 * i + 2];
        const double r = (m.x * (y.x - c0) + m.y * (y.y - c1)) + m.z * (y.z - c2);
        const double J[6] = {c1 * m.z - c2 * m.y, c2 * m.x - c0 * m.z, c0 * m.y - c1 * m.x, s * m.x, s * m.y, s * m.z};
        int e = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) acc[e++] += J[a] * J[b];
        for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * r;
        acc[27] += 0.5 * r * r;
        acc[28] += 1.0;
    }
#pragma unroll
    for (int e = 0; e < 29; ++e) {                 // (unrolled: acc[e] with a run-time e would move the 29 sums to scratch memory)
        red[threadIdx.x] = acc[e];
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0 && partial) {
            partial[29 * (size_t)blockIdx.x + e] = red[0];
        } else if (threadIdx.x == 0 && red[0] != 0.0) {
            if (e < 21) {
                int a = 0, rem = e;
                while (rem >= 6 - a) { rem -= 6 - a; ++a; }
                const int b = a + rem;
                atomicAdd(out + 6 * a + b, red[0]);
                if (a != b) atomicAdd(out + 6 * b + a, red[0]);
            } else {
                atomicAdd(out + 36 + (e - 21), red[0]);
            }
        }
        __syncthreads();
    }
}

// out (44 doubles, see above) = the workgroups' 29 sums added in workgroup order (thread t: rows t, t + 256, ...; then a fixed tree)
__global__ __launch_bounds__(256) void gn_rigid_finish_kernel(const double *__restrict__ partial, int rows, double *__restrict__ out) {
    __shared__ double red[256];
    for (int e = 0; e < 29; ++e) {
        double acc = 0.0;
        for (int b = threadIdx.x; b < rows; b += 256) acc += partial[29 * (size_t)b + e];
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            if (e < 21) {
                int a = 0, rem = e;
                while (rem >= 6 - a) { rem -= 6 - a; ++a; }
                const int b = a + rem;
                out[6 * a + b] = red[0];
                out[6 * b + a] = red[0];
            } else {
                out[36 + (e - 21)] = red[0];
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void top8_insert_s(double (&bd)[kKMaxS], int (&bi)[kKMaxS], double d2, int idx) {
    bool ins = false;                       // once inserted, everything below shifts down: equal distances keep their
#pragma unroll
    for (int i = 0; i < kKMaxS; ++i) {      // arrival order (a stable sort: ties go to the lower node index)
        const bool lt = ins || d2 < bd[i];
        ins = lt;
        const double td = bd[i];
        const int ti = bi[i];
        bd[i] = lt ? d2 : td;
        bi[i] = lt ? idx : ti;
        d2 = lt ? td : d2;
        idx = lt ? ti : idx;
    }
}

// ------------------------------------------------------------------------------- batch warp + correspondences
// Fusion.warp for a batch (core/fusion.py:502-520): nbr == NULL -> only the global m_lw is applied
// (the FusionDM case, dqb_warp(_lw, v) / dqb_warp_normal(_lw, n), fusion_dm.py:230-231).
__global__ __launch_bounds__(256) void warp_points_kernel(const double *__restrict__ verts, const double *__restrict__ norms,
                                                           const int *__restrict__ nbr, int V, int k,
                                                           const double *__restrict__ node_dq,
                                                           const double *__restrict__ node_pos,
                                                           const double *__restrict__ node_w, DQ lw,
                                                           double *__restrict__ out_pos, double *__restrict__ out_nrm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    double px = verts[3 * (size_t)i], py = verts[3 * (size_t)i + 1], pz = verts[3 * (size_t)i + 2];
    double nx = norms ? norms[3 * (size_t)i] : 0.0, ny = norms ? norms[3 * (size_t)i + 1] : 0.0, nz = norms ? norms[3 * (size_t)i + 2] : 0.0;
    if (nbr) {
        int idx[kKMaxS];
#pragma unroll
        for (int j = 0; j < kKMaxS; ++j) idx[j] = j < k ? nbr[(size_t)i * k + j] : 0;
        double bh[8];
        blend_from_indices(node_dq, node_pos, node_w, idx, k, px, py, pz, bh, nullptr, nullptr);
        const D3 x1 = dqb_warp_exact(bh, round_f32(px), round_f32(py), round_f32(pz));
        const D3 n1 = dqb_warp_normal_exact(bh, round_f32(nx), round_f32(ny), round_f32(nz));
        px = x1.x; py = x1.y; pz = x1.z; nx = n1.x; ny = n1.y; nz = n1.z;
    }
    const D3 xp = dqb_warp_exact(lw.q, round_f32(px), round_f32(py), round_f32(pz));
    out_pos[3 * (size_t)i] = xp.x; out_pos[3 * (size_t)i + 1] = xp.y; out_pos[3 * (size_t)i + 2] = xp.z;
    if (out_nrm) {
        const D3 np_ = dqb_warp_normal_exact(lw.q, round_f32(nx), round_f32(ny), round_f32(nz));
        out_nrm[3 * (size_t)i] = np_.x; out_nrm[3 * (size_t)i + 1] = np_.y; out_nrm[3 * (size_t)i + 2] = np_.z;
    }
}

// The selection loop of setupCorrespondences (core/fusion_dm.py:229-244, core/fusion.py:258-276):
// k nearest live vertices of every warped vertex (brute force through LDS tiles, nearest first as
// KDTree.query returns them), best = first neighbour with the smallest cost |wn.(vp - p)| below the
// initial best_cost = 1, kept iff best_cost <= tolerance.
__global__ __launch_bounds__(256) void closest_corr_kernel(const double *__restrict__ wpos, const double *__restrict__ wnrm, int V,
                                                            const double *__restrict__ live, int L, int k, double tolerance,
                                                            double *__restrict__ corr, double *__restrict__ cost_out,
                                                            unsigned char *__restrict__ keep) {
    __shared__ double sp[256 * 3];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool act = i < V;
    const double px = act ? wpos[3 * (size_t)i] : 0.0, py = act ? wpos[3 * (size_t)i + 1] : 0.0, pz = act ? wpos[3 * (size_t)i + 2] : 0.0;
    double bd[kKMaxS];
    int bi[kKMaxS];
#pragma unroll
    for (int j = 0; j < kKMaxS; ++j) { bd[j] = __builtin_huge_val(); bi[j] = -1; }
    for (int base = 0; base < L; base += 256) {
        const int n = min(256, L - base);
        if ((int)threadIdx.x < n) {
            sp[3 * threadIdx.x] = live[3 * (size_t)(base + threadIdx.x)];
            sp[3 * threadIdx.x + 1] = live[3 * (size_t)(base + threadIdx.x) + 1];
            sp[3 * threadIdx.x + 2] = live[3 * (size_t)(base + threadIdx.x) + 2];
        }
        __syncthreads();
        if (act) {
            for (int j = 0; j < n; ++j) {
                const double dx = px - sp[3 * j], dy = py - sp[3 * j + 1], dz = pz - sp[3 * j + 2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < bd[kKMaxS - 1]) top8_insert_s(bd, bi, d2, base + j);
            }
        }
        __syncthreads();
    }
    if (!act) return;
    // A non-finite position has no neighbours (no d2 compares below +inf, the slots keep index -1): no correspondence.
    bool full = true;
#pragma unroll
    for (int j = 0; j < kKMaxS; ++j) full = full && (j >= k || bi[j] >= 0);
    if (!full) {
        corr[3 * (size_t)i] = 0.0; corr[3 * (size_t)i + 1] = 0.0; corr[3 * (size_t)i + 2] = 0.0;
        if (cost_out) cost_out[i] = __builtin_huge_val();
        keep[i] = 0;
        return;
    }
    const double nx = wnrm[3 * (size_t)i], ny = wnrm[3 * (size_t)i + 1], nz = wnrm[3 * (size_t)i + 2];
    double best_cost = 1.0;                                     // fusion_dm.py:234
    int best = bi[0];                                           // lverts[nidxs[0]], :233
#pragma unroll
    for (int j = 0; j < kKMaxS; ++j) {
        if (j < k) {
            const int q = bi[j];
            const double dx = px - live[3 * (size_t)q], dy = py - live[3 * (size_t)q + 1], dz = pz - live[3 * (size_t)q + 2];
            const double c = fabs((nx * dx + ny * dy) + nz * dz);   // :238
            if (c < best_cost) { best_cost = c; best = q; }
        }
    }
    corr[3 * (size_t)i] = live[3 * (size_t)best];
    corr[3 * (size_t)i + 1] = live[3 * (size_t)best + 1];
    corr[3 * (size_t)i + 2] = live[3 * (size_t)best + 2];
    if (cost_out) cost_out[i] = best_cost;
    keep[i] = best_cost <= tolerance ? 1 : 0;                    // :242
}

// ------------------------------------------------------------------------------- deformation-graph maintenance
// Device side of update_graph / construct_graph (reference core/fusion.py:101-123, 201-239).

// Nearest cloud point of every query (KDTree(cloud).query(q), :209-212: a node's anchor vertex): one workgroup per
// query, threads stride over the cloud, lexicographic (d2, index) minimum -- ties go to the lower index.
__global__ __launch_bounds__(256) void nearest_point_kernel(const double *__restrict__ query, int nq, const double *__restrict__ cloud,
                                                             int nc, int *__restrict__ idx_out, double *__restrict__ d2_out) {
    __shared__ double sd[256];
    __shared__ int si[256];
    const int qi = blockIdx.x;
    const double qx = query[3 * (size_t)qi], qy = query[3 * (size_t)qi + 1], qz = query[3 * (size_t)qi + 2];
    double best = __builtin_huge_val();
    int bi = 0x7fffffff;
    for (int j = threadIdx.x; j < nc; j += 256) {
        const double dx = qx - cloud[3 * (size_t)j], dy = qy - cloud[3 * (size_t)j + 1], dz = qz - cloud[3 * (size_t)j + 2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < best) { best = d2; bi = j; }            // (ascending j per thread: the first minimum is kept)
    }
    sd[threadIdx.x] = best; si[threadIdx.x] = bi;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            const double o = sd[threadIdx.x + st];
            const int oi = si[threadIdx.x + st];
            if (o < sd[threadIdx.x] || (o == sd[threadIdx.x] && oi < si[threadIdx.x])) { sd[threadIdx.x] = o; si[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        idx_out[qi] = si[0] == 0x7fffffff ? -1 : si[0];  // (a non-finite query: no thread found a point; d2 = +inf)
        if (d2_out) d2_out[qi] = sd[0];
    }
}

// "unsupported surface point" test of update_graph (:215-219): min over the vertex's knn nodes of |node - v| / w >= 1
__global__ __launch_bounds__(256) void graph_unsupported_kernel(const double *__restrict__ verts, int V, const int *__restrict__ nbr, int k,
                                                                 const double *__restrict__ node_pos, const double *__restrict__ node_w,
                                                                 unsigned char *__restrict__ flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const double px = verts[3 * (size_t)i], py = verts[3 * (size_t)i + 1], pz = verts[3 * (size_t)i + 2];
    double m = __builtin_huge_val();
    for (int j = 0; j < k; ++j) {
        const int gi = nbr[(size_t)i * k + j];
        const double dx = node_pos[3 * gi] - px, dy = node_pos[3 * gi + 1] - py, dz = node_pos[3 * gi + 2] - pz;
        const double r = sqrt((dx * dx + dy * dy) + dz * dz) / node_w[gi];
        m = r < m ? r : m;
    }
    flag[i] = m >= 1.0 ? 1 : 0;
}

// Fusion.dq_blend for a batch (:527-551): the normalised blend of the given nodes' DQs at every point (identity when
// the blend vanishes) -- the DQ a newly inserted node starts from (:222).
__global__ __launch_bounds__(256) void dq_blend_points_kernel(const double *__restrict__ pts, int P, const int *__restrict__ nbr, int k,
                                                               const double *__restrict__ node_dq, const double *__restrict__ node_pos,
                                                               const double *__restrict__ node_w, double *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    int idx[kKMaxS];
#pragma unroll
    for (int j = 0; j < kKMaxS; ++j) idx[j] = j < k ? nbr[(size_t)i * k + j] : 0;
    double bh[8];
    blend_from_indices(node_dq, node_pos, node_w, idx, k, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], bh, nullptr, nullptr);
#pragma unroll
    for (int c = 0; c < 8; ++c) out[8 * (size_t)i + c] = bh[c];
}

// ------------------------------------------------------------------------------- sample setup

// k nearest nodes + Gaussian blend weights of arbitrary sample points.  The 256 samples of a workgroup are
// consecutive band voxels, i.e. spatially coherent: with their bounding box B, any sample's k-th nearest node is no
// farther than the k-th smallest over nodes of maxdist(node, B), so only nodes with mindist(node, B) within that bound
// can be among anyone's k nearest.  Those candidates (kept in node order, so ties resolve as in a full scan) are
// scanned; everything else is skipped.  Same result as brute force, ~10x fewer distance evaluations.
constexpr int kKnnCand = 512;              // candidate capacity in LDS; more -> plain scan of all nodes

__global__ __launch_bounds__(256) void sample_knn_kernel(const double *__restrict__ spos, int S, const double *__restrict__ node_pos,
                                                          const double *__restrict__ node_w, int N, int k,
                                                          int *__restrict__ nbr, double *__restrict__ wts) {
    __shared__ double sp[kKnnCand * 3];
    __shared__ int sid[kKnnCand];
    __shared__ double sred[6][4];
    __shared__ double sbox[6];
    __shared__ int scount[5];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i = blockIdx.x * 256 + tid;
    const bool act = i < S;
    const double px = act ? spos[3 * (size_t)i] : 0.0, py = act ? spos[3 * (size_t)i + 1] : 0.0, pz = act ? spos[3 * (size_t)i + 2] : 0.0;
    // ---- bounding box of the workgroup's samples (the finite ones: a non-finite sample has no neighbours and must not
    //      widen the box of the samples it shares the workgroup with)
    {
        const double big = __builtin_huge_val();
        const bool fin = act && isfinite(px) && isfinite(py) && isfinite(pz);
        double v[6] = {fin ? px : big, fin ? py : big, fin ? pz : big, fin ? -px : big, fin ? -py : big, fin ? -pz : big};   // min of (x, -x)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v[c] = fmin(v[c], __shfl_xor(v[c], o, 64));
            if (lane == 0) sred[c][wv] = v[c];
        }
        __syncthreads();
        if (tid < 6) sbox[tid] = fmin(fmin(sred[tid][0], sred[tid][1]), fmin(sred[tid][2], sred[tid][3]));
        __syncthreads();
    }
    const double lox = sbox[0], loy = sbox[1], loz = sbox[2], hix = -sbox[3], hiy = -sbox[4], hiz = -sbox[5];
    // ---- bound: k-th smallest maxdist^2(node, box); k rounds of "smallest value above the previous one" (ties make the
    //      bound only larger, which is safe)
    auto maxd2 = [&](int n) {
        const double x = node_pos[3 * n], y = node_pos[3 * n + 1], z = node_pos[3 * n + 2];
        const double dx = fmax(fabs(x - lox), fabs(x - hix)), dy = fmax(fabs(y - loy), fabs(y - hiy)), dz = fmax(fabs(z - loz), fabs(z - hiz));
        return (dx * dx + dy * dy) + dz * dz;
    };
    double prev = -1.0;
    for (int r = 0; r < k; ++r) {
        double m = __builtin_huge_val();
        for (int n = tid; n < N; n += 256) {
            const double d = maxd2(n);
            if (d > prev && d < m) m = d;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmin(m, __shfl_xor(m, o, 64));
        if (lane == 0) sred[0][wv] = m;
        __syncthreads();
        prev = fmin(fmin(sred[0][0], sred[0][1]), fmin(sred[0][2], sred[0][3]));
        __syncthreads();
    }
    // (k distinct values were found when N >= k distinct distances exist; with fewer, prev = +inf: every node qualifies)
    const double bound = prev * (1.0 + 1e-12) + 1e-300;
    // ---- candidates: mindist^2(node, box) <= bound, compacted in node order
    int total = 0;
    bool fits = true;
    for (int base = 0; base < N && fits; base += 256) {
        const int n = base + tid;
        bool keep = false;
        if (n < N) {
            const double x = node_pos[3 * n], y = node_pos[3 * n + 1], z = node_pos[3 * n + 2];
            const double dx = fmax(fmax(lox - x, x - hix), 0.0), dy = fmax(fmax(loy - y, y - hiy), 0.0), dz = fmax(fmax(loz - z, z - hiz), 0.0);
            keep = (dx * dx + dy * dy) + dz * dz <= bound;
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) scount[wv] = __popcll(bal);
        __syncthreads();
        int pos = total + __popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wv; ++w) pos += scount[w];
        const int add = scount[0] + scount[1] + scount[2] + scount[3];
        if (total + add > kKnnCand) fits = false;                    // (block-uniform)
        else if (keep) {
            sid[pos] = n;
            sp[3 * pos] = node_pos[3 * n]; sp[3 * pos + 1] = node_pos[3 * n + 1]; sp[3 * pos + 2] = node_pos[3 * n + 2];
        }
        total += add;
        __syncthreads();
    }
    double bd[kKMaxS];
    int bi[kKMaxS];
#pragma unroll
    for (int j = 0; j < kKMaxS; ++j) { bd[j] = __builtin_huge_val(); bi[j] = -1; }
    if (fits) {
        if (act) {
            for (int j = 0; j < total; ++j) {
                const double dx = px - sp[3 * j], dy = py - sp[3 * j + 1], dz = pz - sp[3 * j + 2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < bd[kKMaxS - 1]) top8_insert_s(bd, bi, d2, sid[j]);
            }
        }
    } else {
        for (int base = 0; base < N; base += 256) {                 // too many candidates for LDS: scan all nodes
            const int n = min(256, N - base);
            __syncthreads();
            if (tid < n) {
                sp[3 * tid] = node_pos[3 * (base + tid)];
                sp[3 * tid + 1] = node_pos[3 * (base + tid) + 1];
                sp[3 * tid + 2] = node_pos[3 * (base + tid) + 2];
            }
            __syncthreads();
            if (act) {
                for (int j = 0; j < n; ++j) {
                    const double dx = px - sp[3 * j], dy = py - sp[3 * j + 1], dz = pz - sp[3 * j + 2];
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 < bd[kKMaxS - 1]) top8_insert_s(bd, bi, d2, base + j);
                }
            }
        }
    }
    if (!act) return;
    // A non-finite sample found no neighbour (the slots keep index -1): nodes 0..k-1 with weight 0, as dfh_sample_knn_bricks does.
    bool full = true;
#pragma unroll
    for (int j = 0; j < kKMaxS; ++j) full = full && (j >= k || bi[j] >= 0);
    if (!full) {
        for (int j = 0; j < k; ++j) { nbr[(size_t)i * k + j] = j; wts[(size_t)i * k + j] = 0.0; }
        return;
    }
#pragma unroll
    for (int j = 0; j < kKMaxS; ++j) {
        if (j < k) {
            const int gi = bi[j];
            nbr[(size_t)i * k + j] = gi;
            const double t = sqrt(bd[j]) / (2.0 * node_w[gi]);
            wts[(size_t)i * k + j] = exp(-1.0 * (t * t));
        }
    }
}

// Samples into the order of `order` (the sort by node tuple): positions, normals, node ids and blend weights in one pass.
__global__ __launch_bounds__(256) void permute_samples_kernel(const long *__restrict__ order, int S, int k, const double *__restrict__ pos,
                                                              const double *__restrict__ nrm, const int *__restrict__ nbr,
                                                              const double *__restrict__ wts, double *__restrict__ pos_o,
                                                              double *__restrict__ nrm_o, int *__restrict__ nbr_o, double *__restrict__ wts_o) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    const size_t src = (size_t)order[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        pos_o[3 * (size_t)i + c] = pos[3 * src + c];
        nrm_o[3 * (size_t)i + c] = nrm[3 * src + c];
    }
    for (int j = 0; j < k; ++j) {
        nbr_o[(size_t)i * k + j] = nbr[src * k + j];
        wts_o[(size_t)i * k + j] = wts[src * k + j];
    }
}

}  // namespace dfh

// =================================================================================== C ABI
extern "C" {

int dfh_residual_rigid(const double *verts, const double *normals, const double *corr, int n, const double x[8],
                       double *out, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(n >= 0, "dfh_residual_rigid: negative count");
    if (n == 0) return DFH_OK;
    DFH_REQUIRE(verts && normals && corr && x && out, "dfh_residual_rigid: null pointer");
    DQ q;
    for (int i = 0; i < 8; ++i) q.q[i] = x[i];
    hipLaunchKernelGGL(residual_rigid_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, verts, normals, corr, n, q, out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_gn_build_rigid(const double *verts, const double *normals, const double *corr, const unsigned char *valid, int n,
                       const double x[8], double *out44, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(n >= 0 && x && out44, "dfh_gn_build_rigid: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    DFH_HIP_CHECK(hipMemsetAsync(out44, 0, sizeof(double) * 44, s));
    if (n == 0) return DFH_OK;
    DFH_REQUIRE(verts && normals && corr, "dfh_gn_build_rigid: null pointer");
    DQ q;
    for (int i = 0; i < 8; ++i) q.q[i] = x[i];
    int blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    // per-workgroup sums in stream-ordered scratch, added in a fixed order by a second launch: the same bits every run.
    // (No scratch -- allocation refused, e.g. inside a stream capture without pool support: atomics, last bits may vary.)
    double *partial = nullptr;
    if (on(opt().rigid_atomic) || hipMallocAsync(reinterpret_cast<void **>(&partial), sizeof(double) * 29 * (size_t)blocks, s) != hipSuccess) {
        (void)hipGetLastError();
        partial = nullptr;
    }
    hipLaunchKernelGGL(gn_build_rigid_kernel, dim3(blocks), dim3(256), 0, s, verts, normals, corr, valid, n, q, out44, partial);
    if (partial) {
        hipLaunchKernelGGL(gn_rigid_finish_kernel, dim3(1), dim3(256), 0, s, partial, blocks, out44);
        DFH_HIP_CHECK(hipFreeAsync(partial, s));
    }
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_residual_data(const double *verts, const double *normals, const double *corr, const int *nbr, int n_verts,
                      int knn, const double *node_dq, const double *node_pos, const double *node_w, int n_nodes,
                      const double lw_dq[8], double *out, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(n_verts >= 0 && n_nodes >= 1, "dfh_residual_data: bad sizes");
    DFH_REQUIRE(knn >= 1 && knn <= kKMaxS, "dfh_residual_data: knn=%d outside [1,%d]", knn, kKMaxS);
    if (n_verts == 0) return DFH_OK;
    DFH_REQUIRE(verts && normals && corr && nbr && node_dq && node_pos && node_w && lw_dq && out, "dfh_residual_data: null pointer");
    DQ q;
    for (int i = 0; i < 8; ++i) q.q[i] = lw_dq[i];
    hipLaunchKernelGGL(residual_data_kernel, dim3((n_verts + 255) / 256), dim3(256), 0, (hipStream_t)stream, verts, normals,
                       corr, nbr, n_verts, knn, node_dq, node_pos, node_w, q, out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_residual_reg(const int *node_nbr, int n_nodes, int knn, const double *node_dq, const double *node_pos,
                     const double *node_w, double rw, double *out, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(n_nodes >= 0 && knn >= 1 && knn <= kKMaxS, "dfh_residual_reg: bad sizes");
    if (n_nodes == 0) return DFH_OK;
    DFH_REQUIRE(node_nbr && node_dq && node_pos && node_w && out, "dfh_residual_reg: null pointer");
    const int n = n_nodes * knn;
    hipLaunchKernelGGL(residual_reg_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, node_nbr, n_nodes, knn,
                       node_dq, node_pos, node_w, rw, out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_warp_points(const double *verts, const double *normals, const int *nbr, int n_verts, int knn, const double *node_dq,
                    const double *node_pos, const double *node_w, int n_nodes, const double lw_dq[8], double *out_pos,
                    double *out_nrm, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(n_verts >= 0, "dfh_warp_points: negative count");
    if (n_verts == 0) return DFH_OK;
    DFH_REQUIRE(verts && lw_dq && out_pos, "dfh_warp_points: null pointer");
    DFH_REQUIRE((normals == nullptr) == (out_nrm == nullptr) || normals, "dfh_warp_points: out_nrm needs normals");
    if (nbr) {
        DFH_REQUIRE(knn >= 1 && knn <= kKMaxS && n_nodes >= 1 && node_dq && node_pos && node_w, "dfh_warp_points: bad graph arguments");
    }
    DQ q;
    for (int i = 0; i < 8; ++i) q.q[i] = lw_dq[i];
    hipLaunchKernelGGL(warp_points_kernel, dim3((n_verts + 255) / 256), dim3(256), 0, (hipStream_t)stream, verts, normals, nbr,
                       n_verts, knn, node_dq, node_pos, node_w, q, out_pos, normals ? out_nrm : nullptr);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_closest_correspondences(const double *warped_pos, const double *warped_nrm, int n_verts, const double *live_verts,
                                int n_live, int knn, double tolerance, double *corr_out, double *cost_out,
                                unsigned char *keep_out, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(n_verts >= 0 && knn >= 1 && knn <= kKMaxS, "dfh_closest_correspondences: bad sizes");
    DFH_REQUIRE(n_live >= knn, "dfh_closest_correspondences: %d live vertices < knn=%d", n_live, knn);
    if (n_verts == 0) return DFH_OK;
    DFH_REQUIRE(warped_pos && warped_nrm && live_verts && corr_out && keep_out, "dfh_closest_correspondences: null pointer");
    hipLaunchKernelGGL(closest_corr_kernel, dim3((n_verts + 255) / 256), dim3(256), 0, (hipStream_t)stream, warped_pos, warped_nrm,
                       n_verts, live_verts, n_live, knn, tolerance, corr_out, cost_out, keep_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_nearest_points(const double *query, int n_query, const double *cloud, int n_cloud, int *idx_out, double *d2_out, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(n_query >= 0 && n_cloud >= 1, "dfh_nearest_points: bad sizes");
    if (n_query == 0) return DFH_OK;
    DFH_REQUIRE(query && cloud && idx_out, "dfh_nearest_points: null pointer");
    hipLaunchKernelGGL(nearest_point_kernel, dim3(n_query), dim3(256), 0, (hipStream_t)stream, query, n_query, cloud, n_cloud, idx_out, d2_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_graph_unsupported(const double *verts, int n_verts, const int *nbr, int knn, const double *node_pos, const double *node_w,
                          int n_nodes, unsigned char *flag_out, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(n_verts >= 0 && knn >= 1 && knn <= kKMaxS && n_nodes >= 1, "dfh_graph_unsupported: bad sizes");
    if (n_verts == 0) return DFH_OK;
    DFH_REQUIRE(verts && nbr && node_pos && node_w && flag_out, "dfh_graph_unsupported: null pointer");
    hipLaunchKernelGGL(graph_unsupported_kernel, dim3((n_verts + 255) / 256), dim3(256), 0, (hipStream_t)stream, verts, n_verts, nbr, knn,
                       node_pos, node_w, flag_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_dq_blend_points(const double *points, int n_points, const int *nbr, int knn, const double *node_dq, const double *node_pos,
                        const double *node_w, int n_nodes, double *dq_out, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(n_points >= 0 && knn >= 1 && knn <= kKMaxS && n_nodes >= 1, "dfh_dq_blend_points: bad sizes");
    if (n_points == 0) return DFH_OK;
    DFH_REQUIRE(points && nbr && node_dq && node_pos && node_w && dq_out, "dfh_dq_blend_points: null pointer");
    hipLaunchKernelGGL(dq_blend_points_kernel, dim3((n_points + 255) / 256), dim3(256), 0, (hipStream_t)stream, points, n_points, nbr, knn,
                       node_dq, node_pos, node_w, dq_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_sample_knn(const double *sample_pos, int n_samples, const double *node_pos, const double *node_w, int n_nodes,
                   int knn, int *nbr_out, double *weights_out, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(n_samples >= 0 && knn >= 1 && knn <= kKMaxS && n_nodes >= knn, "dfh_sample_knn: bad sizes");
    if (n_samples == 0) return DFH_OK;
    DFH_REQUIRE(sample_pos && node_pos && node_w && nbr_out && weights_out, "dfh_sample_knn: null pointer");
    hipLaunchKernelGGL(sample_knn_kernel, dim3((n_samples + 255) / 256), dim3(256), 0, (hipStream_t)stream, sample_pos,
                       n_samples, node_pos, node_w, n_nodes, knn, nbr_out, weights_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

int dfh_permute_samples(const long *order, int n_samples, int knn, const double *pos, const double *nrm, const int *nbr,
                        const double *weights, double *pos_out, double *nrm_out, int *nbr_out, double *weights_out, void *stream) {
    using namespace dfh;
    DFH_REQUIRE(n_samples >= 0 && knn >= 1 && knn <= kKMaxS, "dfh_permute_samples: bad sizes");
    if (n_samples == 0) return DFH_OK;
    DFH_REQUIRE(order && pos && nrm && nbr && weights && pos_out && nrm_out && nbr_out && weights_out, "dfh_permute_samples: null pointer");
    hipLaunchKernelGGL(permute_samples_kernel, dim3((n_samples + 255) / 256), dim3(256), 0, (hipStream_t)stream, order, n_samples, knn, pos,
                       nrm, nbr, weights, pos_out, nrm_out, nbr_out, weights_out);
    DFH_HIP_CHECK(hipGetLastError());
    return DFH_OK;
}

}  // extern "C"
