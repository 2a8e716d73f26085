/*
 * drcvar_loop_route.h — C ABI of the route library (libdrcvar_loop_route.so): a batch of
 * receding-horizon loops whose REFERENCE PATH is each problem's own, beside its own metric, risk
 * parameters and draws shared by choice (drcvar_loop_metric.h, drcvar_loop_risk.h).  Two entries:
 * the sampled halfspaces about each problem's own ego path, and the advance that refills each
 * problem's reference window and fallback inputs from its own paths.  Built beside the engine
 * library from csrc/drcvar_sampled.hip and csrc/drcvar_step.hip (each compiled once more with
 * DRCVAR_LOOP_ROUTE_LIBRARY, linked into one library).  The engine library's symbol list (33
 * symbols, ABI 3) and those of the loop, loop-evaluation, predicted-ego, risk-table and metric
 * libraries are unchanged by it.  Conventions, return codes and drcvar_step_state:
 * drcvar_sampling.h, drcvar_mpc.h.
 */
#ifndef DRCVAR_LOOP_ROUTE_H
#define DRCVAR_LOOP_ROUTE_H

#include <stdint.h>

#include "drcvar_mpc.h"
#include "drcvar_sampling.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * drcvar_sampled_halfspaces_f64_metric (drcvar_loop_metric.h) with an ego path per problem: the
 * arguments of that entry in their order, and after ego_stride
 *
 *   ego_problem_stride   doubles from problem b's ego path to problem b + 1's
 *
 * The ego of window unit (o, t) of problem b = o / n_obstacles_per_problem is
 * ego_path + b * ego_problem_stride + c(step + t) * ego_stride (two adjacent doubles), c = clamp
 * to [0, path_steps - 1].  The caller keeps ego_path readable at every such address for
 * b < n_obstacles / n_obstacles_per_problem; the paths are written before the launch on the same
 * stream or earlier, never by it.
 *
 * Defining property.  For every problem b the launch writes into that problem's rows of `out`,
 * `status` and `selected` the bytes drcvar_sampled_halfspaces_f64_metric writes for the unit
 * window [b O T, (b + 1) O T) (clipped to this launch's window) with ego_path + b *
 * ego_problem_stride as its ego path and all other arguments equal.  ego_problem_stride == 0 is
 * the metric entry, byte for byte.
 *
 * Host checks: ego_problem_stride < 0: DRCVAR_ERR_INVALID_ARGUMENT; above 2^40:
 * DRCVAR_ERR_UNSUPPORTED; then everything drcvar_sampled_halfspaces_f64_metric rejects, with the
 * same code and in its order.  unit_count == 0: DRCVAR_OK, nothing is launched and no pointer is
 * looked at.  Asynchronous on `stream`, no allocation, no synchronisation; capturable.
 */
int drcvar_sampled_halfspaces_f64_route(
    const double* nominal_path, int64_t n_obstacles, int64_t path_steps, int64_t nom_so,
    int64_t nom_st, int64_t n_steps, int64_t unit_begin, int64_t unit_count, int64_t n_samples,
    double l00, double l10, double l11, uint64_t seed, const drcvar_step_state* state,
    int32_t zero_first_step, const double* ego_path, int64_t ego_stride,
    int64_t ego_problem_stride, int64_t n_obstacles_per_problem, const void* table,
    int64_t draw_period, const int32_t* metric, double* out, int32_t* status, double* selected,
    void* stream);

/*
 * drcvar_mpc_step_advance_batch_f64 (drcvar_loop.h) with reference paths per problem: the
 * arguments of that entry in their order, and after path_steps
 *
 *   x_ref_problem_stride, u_ref_problem_stride   doubles from problem b's path to problem b + 1's
 *
 * Problem b reads x_ref_path + b * x_ref_problem_stride ([path_steps, nx], dense rows) and
 * u_ref_path + b * u_ref_problem_stride ([path_steps, nu]); path_steps, step_begin and log_rows
 * are shared.
 *
 * Defining property.  After the launch every byte of every buffer is what n_problems calls of the
 * single entry drcvar_mpc_step_advance_f64 (drcvar_mpc.h) on problem b's slices, with problem b's
 * paths, would leave.  Both strides 0 is the batch entry, byte for byte.
 *
 * Host checks: n_problems < 0: DRCVAR_ERR_INVALID_ARGUMENT; n_problems == 0: DRCVAR_OK, nothing is
 * launched and no other argument is looked at; a stride < 0: DRCVAR_ERR_INVALID_ARGUMENT; then the
 * checks of the batch entry; a stride above 2^40: DRCVAR_ERR_UNSUPPORTED, beside n_problems above
 * 2^31 - 1 (after every invalid argument: an invalid call stays invalid).  Asynchronous on
 * `stream`, no allocation, no synchronisation; capturable.
 */
int drcvar_mpc_step_advance_batch_route_f64(
    const drcvar_mpc_model* model, int64_t n_problems, const double* x_out, const double* u_out,
    const double* info, const double* x_ref_path, const double* u_ref_path, int64_t path_steps,
    int64_t x_ref_problem_stride, int64_t u_ref_problem_stride, const double* disturbance,
    int64_t step_begin, int64_t log_rows, double* x_log, double* u_log, double* info_log,
    double* x0, double* x_ref_win, double* u_fallback, double* last_u, int32_t* have_last,
    drcvar_step_state* state, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRCVAR_LOOP_ROUTE_H */
