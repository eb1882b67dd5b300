// The volume data term's cell evaluation, stated once: steps 2-7 of the definition of dfh_gn_associate_volume
// (include/dfusion_hip.h) for one warped sample.  Run by associate_volume_kernel (dfh_associate_volume.hip), by the volume mode
// of the data-row kernel (dfh_solve.hip: gn_build_data_kernel) and by the volume mode of the rigid-mode rows kernel
// (dfh_gn_global.hip: gn_global_rows_kernel) -- the same operations in the same order, so the three give the same bits -- and
// the argument checks the entry points of the volume term share.
#pragma once
#include "dfh_dq.h"

#include <cmath>

namespace dfh {

struct VolAssocParams {
    DQ lw;
    double value_to_vox, band, max_dist2, min_grad2;   // max_dist2 <= 0: no gate
    int res[3];
};

// two z-adjacent voxels: the pair is only element-aligned (a cell starts at any z), which the load is told
template <typename LiveT>
struct LivePair { LiveT lo, hi; };

template <typename LiveT>
__device__ __forceinline__ LivePair<LiveT> load_pair(const LiveT *__restrict__ p) {
    LivePair<LiveT> v;
    __builtin_memcpy(&v, p, sizeof(v));                // one global_load_dwordx2 (float) / dwordx4 (double), alignment sizeof(LiveT)
    return v;
}

// What a kernel that associates against a volume inside another computation is given (vol_assoc_args below fills it).
struct VolAssocArgs {
    VolAssocParams vp;
    const void *live;           // the whole live volume, of the type the kernel is instantiated for
};

// xp: the warped sample (step 1 is the caller's).  c <- the correspondence, (0, 0, 0) when the sample is not usable; returns
// usable.  Every lane that calls this loads: lanes outside the grid read cell (0,0,0) instead of branching round the loads (no
// divergence, one exit) and are discarded -- a caller whose lane has NO sample must not call it.
template <typename LiveT>
__device__ __forceinline__ bool associate_volume_cell(const LiveT *__restrict__ live, const VolAssocParams &p, const D3 &xp, double (&c)[3]) {
    // 2. in grid: decided on the doubles (NaN and +-inf fail the comparisons), before any conversion to int
    const bool in_grid = xp.x >= 0.0 && xp.x < (double)(p.res[0] - 1) && xp.y >= 0.0 && xp.y < (double)(p.res[1] - 1) &&
                         xp.z >= 0.0 && xp.z < (double)(p.res[2] - 1);
    const double X0 = in_grid ? xp.x : 0.0, X1 = in_grid ? xp.y : 0.0, X2 = in_grid ? xp.z : 0.0;   // (outside: cell (0,0,0), discarded)
    const double fl0 = floor(X0), fl1 = floor(X1), fl2 = floor(X2);
    const int i0 = (int)fl0, i1 = (int)fl1, i2 = (int)fl2;          // 0 <= ia <= res[a] - 2
    const double f0 = X0 - fl0, f1 = X1 - fl1, f2 = X2 - fl2;
    // 3. corners: the standard trilinear cell, four z-adjacent pairs, all requested before the first use (the cell index in
    // size_t: 512^3 is 134 M voxels, a float64 volume of that size 1 GB)
    const size_t sy = (size_t)p.res[2], sx = (size_t)p.res[1] * sy;
    const LiveT *cell = live + ((size_t)i0 * sx + (size_t)i1 * sy + (size_t)i2);
    const LivePair<LiveT> r00 = load_pair(cell), r01 = load_pair(cell + sy), r10 = load_pair(cell + sx), r11 = load_pair(cell + sx + sy);
    const double u000 = (double)r00.lo * p.value_to_vox, u001 = (double)r00.hi * p.value_to_vox;
    const double u010 = (double)r01.lo * p.value_to_vox, u011 = (double)r01.hi * p.value_to_vox;
    const double u100 = (double)r10.lo * p.value_to_vox, u101 = (double)r10.hi * p.value_to_vox;
    const double u110 = (double)r11.lo * p.value_to_vox, u111 = (double)r11.hi * p.value_to_vox;
    // 4. band (strict; a NaN corner fails)
    const bool in_band = fabs(u000) < p.band && fabs(u001) < p.band && fabs(u010) < p.band && fabs(u011) < p.band &&
                         fabs(u100) < p.band && fabs(u101) < p.band && fabs(u110) < p.band && fabs(u111) < p.band;
    // 5. value and gradient of the interpolant
    const double dz00 = u001 - u000, dz01 = u011 - u010, dz10 = u101 - u100, dz11 = u111 - u110;
    const double e00 = u000 + f2 * dz00, e01 = u010 + f2 * dz01, e10 = u100 + f2 * dz10, e11 = u110 + f2 * dz11;
    const double dy0 = e01 - e00, dy1 = e11 - e10;
    const double h0 = e00 + f1 * dy0, h1 = e10 + f1 * dy1;
    const double g0 = h1 - h0;
    const double s = h0 + f0 * g0;
    const double g1 = dy0 + f0 * (dy1 - dy0);
    const double m0 = dz00 + f1 * (dz01 - dz00), m1 = dz10 + f1 * (dz11 - dz10);
    const double g2 = m0 + f0 * (m1 - m0);
    // 6. gradient and gate (G > 0 always: t = s / G)
    const double G = (g0 * g0 + g1 * g1) + g2 * g2;
    bool ok = in_grid && in_band && G >= p.min_grad2 && G > 0.0;
    if (p.max_dist2 > 0.0) ok = ok && s * s <= p.max_dist2 * G;
    // 7. one Newton step onto the zero level set
    const double t = s / G;
    c[0] = ok ? xp.x - t * g0 : 0.0;
    c[1] = ok ? xp.y - t * g1 : 0.0;
    c[2] = ok ? xp.z - t * g2 : 0.0;
    return ok;
}

// ------------------------------------------------------------------------------- host side
// What every entry point of the volume term checks of its term; `fused`: the cell is evaluated inside the data-row kernel, which
// reads float32 volumes only.
inline int check_volume_term(const char *what, const dfh_gn_volume_term *term, bool fused) {
    DFH_REQUIRE(term, "%s: null volume term", what);
    const dfh_gn_volume_term &v = *term;
    DFH_REQUIRE(v.live.data, "%s: null live volume", what);
    DFH_REQUIRE(v.live.dtype == DFH_F32 || v.live.dtype == DFH_F64, "%s: bad live dtype %d", what, v.live.dtype);
    DFH_REQUIRE(!fused || v.live.dtype == DFH_F32, "%s: the fused association needs a float32 live volume", what);
    DFH_REQUIRE(v.live.res[0] >= 2 && v.live.res[1] >= 2 && v.live.res[2] >= 2, "%s: bad grid %dx%dx%d (a cell needs 2 voxels per axis)",
                what, v.live.res[0], v.live.res[1], v.live.res[2]);
    DFH_REQUIRE(std::isfinite(v.value_to_vox) && v.value_to_vox != 0.0, "%s: value_to_vox must be finite and non-zero", what);
    DFH_REQUIRE(v.band > 0.0, "%s: band must be > 0", what);                       // (NaN fails)
    DFH_REQUIRE(v.min_grad >= 0.0, "%s: min_grad must be >= 0", what);             // (NaN fails)
    DFH_REQUIRE(!std::isnan(v.max_dist), "%s: max_dist is NaN", what);
    return DFH_OK;
}

// The cell evaluation's kernel arguments, from the problem's lw_dq and a checked term.
inline VolAssocParams vol_assoc_params(const dfh_gn_problem &q, const dfh_gn_volume_term &v) {
    VolAssocParams p;
    for (int c = 0; c < 8; ++c) p.lw.q[c] = q.lw_dq[c];
    p.value_to_vox = v.value_to_vox;
    p.band = v.band;
    p.max_dist2 = v.max_dist > 0.0 ? v.max_dist * v.max_dist : 0.0;
    p.min_grad2 = v.min_grad * v.min_grad;
    for (int a = 0; a < 3; ++a) p.res[a] = v.live.res[a];
    return p;
}

inline VolAssocArgs vol_assoc_args(const dfh_gn_problem &q, const dfh_gn_volume_term &v) {
    VolAssocArgs va;
    va.vp = vol_assoc_params(q, v);
    va.live = v.live.data;
    return va;
}

}  // namespace dfh
