/*
 * drcvar_loop_pred.h — C ABI of the predicted-ego library (libdrcvar_loop_pred.so): the sampled
 * halfspaces of receding-horizon loops linearised about each loop's OWN predicted path, built
 * beside the engine library from csrc/drcvar_sampled.hip (compiled once more with
 * DRCVAR_LOOP_PRED_LIBRARY).  The engine library's symbol list (33 symbols, ABI 3), the loop
 * library's (drcvar_loop.h) and the loop-evaluation library's (drcvar_loop_eval.h) are unchanged
 * by it.  Conventions, return codes and drcvar_step_state: drcvar_sampling.h.
 */
#ifndef DRCVAR_LOOP_PRED_H
#define DRCVAR_LOOP_PRED_H

#include <stdint.h>

#include "drcvar_sampling.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * drcvar_sampled_halfspaces_f64_dev with a predicted ego: one launch covers B problems of
 * n_obstacles_per_problem = O obstacles each (n_obstacles = B O obstacle paths in nominal_path)
 * over a window of T = n_steps rows, and the separating direction of a unit is taken from its own
 * problem's state and prediction instead of one shared ego path.
 *
 * Unit u = (b O + o) T + t.  The unit numbering, the Philox counters, the stream words read from
 * `state`, zero_first_step at t = 0 and the clamp of the step are drcvar_sampled_halfspaces_f64_dev's,
 * so the draws are bit for bit its draws, and the nominal row of the unit is c(state->step + t),
 * c(r) = min(max(r, 0), path_steps - 1).  The ego is
 *
 *   xs  = (t == 0) ? x0[b, :] : pred[b, min(t + shift, pred_rows - 1), :]
 *   ego = c_out xs          each coordinate an fma chain over j = 0 .. n_states - 1 from +0.0
 *                           (as drcvar_loop_clearance_f64 forms it)
 *
 * For every problem b the record bytes and status words of its units are those of
 * drcvar_sampled_halfspaces_f64 on the gathered window [O, T, 2] of its obstacles with that ego
 * [T, 2], unit_begin = b O T, unit_count = O T and the state's stream offset.  A non-finite x0 or
 * pred row reaches the record and the status word the way a non-finite ego does there, and touches
 * the units of its own problem and row alone.
 *
 * With shift = 1 and pred the solver's x_out of the previous control step, the ego of window row t
 * is the loop's own predicted position at the path time of the obstacle row it is paired with; at
 * t = 0 it is the state actually reached.  shift = 0 linearises about an answer for the same
 * window (a second pass of the same step).
 *
 *   nominal_path [B O, path_steps, 2]: obstacle stride nom_so, row stride nom_st (doubles),
 *                                      adjacent coordinates
 *   x0 [B, n_states] dense; pred [B, pred_rows, n_states] dense: device memory, written by earlier
 *                                      work on the same stream, never by this launch
 *   c_out [2, n_states] row-major HOST memory, copied into the kernel arguments at call time
 *   state: one 16-byte record, 16-byte aligned (read when the kernel runs); out [unit_count, 8];
 *   status [unit_count] or NULL
 *
 * Host checks: n_states outside 1..8, n_obstacles_per_problem < 1, pred_rows < 1, shift outside
 * {0, 1}, n_obstacles not a multiple of n_obstacles_per_problem, a null x0, pred or c_out (when
 * something would be launched), a unit window outside [0, B O T), and everything
 * drcvar_sampled_halfspaces_f64_dev rejects for the arguments the two entries share (a null
 * nominal_path, out or state, a state that is not 16-byte aligned, path_steps < 1, ...):
 * DRCVAR_ERR_INVALID_ARGUMENT.  Its limits (n_samples, the grid): DRCVAR_ERR_UNSUPPORTED.
 * unit_count == 0: DRCVAR_OK, nothing is launched.  Asynchronous on `stream`, no allocation, no
 * synchronisation; capturable.
 */
int drcvar_sampled_halfspaces_f64_pred(
    const double* nominal_path, int64_t n_obstacles, int64_t path_steps, int64_t nom_so,
    int64_t nom_st, int64_t n_steps, int64_t unit_begin, int64_t unit_count, int64_t n_samples,
    double l00, double l10, double l11, uint64_t seed, const drcvar_step_state* state,
    int32_t zero_first_step, int64_t n_obstacles_per_problem, const double* x0, const double* pred,
    int64_t pred_rows, int32_t n_states, const double* c_out, int32_t shift, double robot_radius,
    double obstacle_radius, double alpha, double delta, double epsilon, double* out,
    int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRCVAR_LOOP_PRED_H */
