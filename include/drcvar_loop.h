/*
 * drcvar_loop.h — C ABI of the loop library (libdrcvar_loop.so): entries for batches of
 * receding-horizon loops, built beside the engine library from csrc/drcvar_step.hip.  The engine
 * library's own symbol list (include/drcvar_halfspace.h, drcvar_mpc.h, drcvar_sampling.h,
 * drcvar_exchange.h: 33 symbols, ABI 3) is unchanged by it.  Conventions as in drcvar_mpc.h.
 */
#ifndef DRCVAR_LOOP_H
#define DRCVAR_LOOP_H

#include <stdint.h>

#include "drcvar_mpc.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Close one control step of n_problems receding-horizon loops that advance in lockstep, in one
 * launch (one workgroup per problem, csrc/drcvar_step.hip): for b = 0 .. n_problems - 1 exactly
 * steps 1-7 of drcvar_mpc_step_advance_f64 (drcvar_mpc.h) on problem b's slices, with state[b],
 * info[b, :], have_last[b] and disturbance[b, :, :] — after the launch every byte of every buffer
 * is what n_problems calls of the single entry would leave.  The paths, step_begin and log_rows are
 * shared.
 *
 * ONE STATE PER PROBLEM: `state` is an array of n_problems 16-byte records (base 16-byte aligned)
 * and workgroup b reads and writes state[b] only.  One shared record written by one workgroup
 * would race with the other workgroups' reads of it inside the launch; per-problem records need no
 * atomics and no ordering between workgroups, only the stream's order of launches.  Each problem
 * follows its own state[b]: the entry does not require the records to be equal.  (A lockstep
 * caller keeps them equal, and hands state[0] to drcvar_sampled_halfspaces_f64_dev, whose one launch
 * then draws the n_problems * n_obstacles obstacles of all problems: unit
 * (b * n_obstacles + o) * H + t.)
 *
 *   x_out [B, H+1, nx], u_out [B, H, nu], info [B, DRCVAR_MPC_INFO_WIDTH]   the solver's outputs
 *   x_ref_path [path_steps, nx], u_ref_path [path_steps, nu]               shared by all problems
 *   disturbance [B, log_rows, nx] or NULL
 *   x_log [B, log_rows + 1, nx], u_log [B, log_rows, nu], info_log [B, log_rows, DRCVAR_MPC_INFO_WIDTH]
 *   x0 [B, nx], x_ref_win [B, H+1, nx], u_fallback [B, H, nu], last_u [B, H, nu], have_last [B],
 *   state [B]              all dense, B = n_problems; none may overlap another or an input.
 * Host checks: n_problems < 0: DRCVAR_ERR_INVALID_ARGUMENT; n_problems == 0: DRCVAR_OK, nothing is
 * launched and no other argument is looked at; then the checks of the single entry; n_problems
 * above 2^31 - 1 (the grid's limit): DRCVAR_ERR_UNSUPPORTED.  Asynchronous on `stream`, no
 * allocation, no synchronisation.
 */
int drcvar_mpc_step_advance_batch_f64(const drcvar_mpc_model* model, int64_t n_problems,
                                      const double* x_out, const double* u_out, const double* info,
                                      const double* x_ref_path, const double* u_ref_path,
                                      int64_t path_steps, const double* disturbance,
                                      int64_t step_begin, int64_t log_rows, double* x_log,
                                      double* u_log, double* info_log, double* x0,
                                      double* x_ref_win, double* u_fallback, double* last_u,
                                      int32_t* have_last, drcvar_step_state* state, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRCVAR_LOOP_H */
