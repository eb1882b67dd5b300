// The two PCG internals (dfh_pcg.hip) that dfh_gn_solve (dfh_solve.hip) needs to queue a frame's iterations back to back.
#pragma once
#include <cstddef>

namespace dfh {

// dfh_pcg_solve / dfh_pcg_solve_update (update_dq: the twist update after the solve, all or nothing); precleared: the caller
// has already zeroed pcg_zero_range's part of the workspace on this stream
int pcg_solve_impl(const int *row_ptr, const int *col, double *vals, const double *rhs, int n_nodes, int iters,
                   double lm_abs, double lm_rel, double *x_out, void *workspace, size_t workspace_bytes, double *update_dq,
                   double update_step, void *stream, bool precleared = false);

// the part of the workspace a solve expects all-zero at its start: the multi-launch path's first direction and its scalars, the
// persistent kernel's scalars, reduction slots and hand-off ring (zero bits = "not yet published")
void pcg_zero_range(void *workspace, int n_nodes, int iters, double **begin, size_t *count);

}  // namespace dfh
