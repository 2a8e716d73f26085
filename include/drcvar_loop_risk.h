/*
 * drcvar_loop_risk.h — C ABI of the risk-table library (libdrcvar_loop_risk.so): the sampled
 * halfspaces of a batch of receding-horizon loops whose risk parameters (alpha, delta, epsilon)
 * are each problem's OWN, and whose draws are shared between problems by choice.  Built beside the
 * engine library from csrc/drcvar_sampled.hip (compiled once more with DRCVAR_LOOP_RISK_LIBRARY).
 * The engine library's symbol list (33 symbols, ABI 3), the loop library's (drcvar_loop.h), the
 * loop-evaluation library's (drcvar_loop_eval.h) and the predicted-ego library's
 * (drcvar_loop_pred.h) are unchanged by it.  Conventions, return codes and drcvar_step_state:
 * drcvar_sampling.h.
 */
#ifndef DRCVAR_LOOP_RISK_H
#define DRCVAR_LOOP_RISK_H

#include <stdint.h>

#include "drcvar_sampling.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The risk table: one opaque row per problem, drcvar_risk_table_row_bytes() bytes each (a multiple
 * of 16).  Row b holds exactly what the launch-uniform entries pass to their kernel for the
 * scalars (robot_radius, obstacle_radius, alpha[b], delta[b], epsilon[b]) at n_samples: the rank
 * of the order statistic, 1 / (alpha N), the histogram window of the launch plan that n_samples
 * selects, and the two unbounded exits.  A table is therefore filled FOR one n_samples.
 */
int64_t drcvar_risk_table_row_bytes(void);

/*
 * Writes n_problems rows into table_host, HOST memory of table_bytes bytes; the caller copies them
 * to the device once (16-byte aligned there).  alpha, delta, epsilon: host arrays [n_problems].
 * Rows with equal scalars are equal bytes (the padding is zero).
 *
 * n_problems < 0, a null pointer (with n_problems > 0), table_bytes < n_problems * row bytes, or a
 * row the launch-uniform entries would reject (a non-finite scalar, alpha <= 0):
 * DRCVAR_ERR_INVALID_ARGUMENT, and nothing is written.  alpha > 1 and epsilon < 0 are legal rows:
 * the kernel's UNBOUNDED and DR_UNBOUNDED exits.  n_samples outside 1..DRCVAR_MAX_SAMPLES:
 * DRCVAR_ERR_UNSUPPORTED.  n_problems == 0: DRCVAR_OK.  No device call is made.
 */
int drcvar_risk_table_fill(const double* alpha, const double* delta, const double* epsilon,
                           int64_t n_problems, double robot_radius, double obstacle_radius,
                           int64_t n_samples, void* table_host, int64_t table_bytes);

/*
 * drcvar_sampled_halfspaces_f64_dev with a risk table: one launch covers B problems of
 * n_obstacles_per_problem = O obstacles each (n_obstacles = B O obstacle paths in nominal_path)
 * over a window of T = n_steps rows.  Unit u = (b O + o) T + t takes everything
 * drcvar_sampled_halfspaces_f64_dev's unit u takes (the nominal row c(state->step + t), the shared
 * ego_path, the stream words read from `state`, zero_first_step at t = 0) but
 *
 *   its risk parameters are row b of `table`, and
 *   its Philox counters are those of the draw unit  u_d = ((b mod D) O + o) T + t,
 *   D = draw_period >= 1.
 *
 * D >= B: u_d = u, the draws of drcvar_sampled_halfspaces_f64_dev.  D = 1: every problem meets
 * problem 0's draws.  B = S D with the problems ordered b = s D + r: S settings meet the same D
 * replicate draws (common random numbers).
 *
 * For every problem b the record bytes and status words of its O T units are those of
 * drcvar_sampled_halfspaces_f64 called with a nominal tensor whose obstacle rows (b mod D) O ..
 * + O are problem b's gathered window (earlier rows arbitrary), the gathered ego window,
 * unit_begin = (b mod D) O T, unit_count = O T, the state's stream offset and the scalars
 * (robot_radius, obstacle_radius, alpha[b], delta[b], epsilon[b]) the table was filled with.
 *
 *   nominal_path [B O, path_steps, 2]: obstacle stride nom_so, row stride nom_st (doubles),
 *                                      adjacent coordinates
 *   ego_path [path_steps, 2]: row stride ego_stride
 *   table: DEVICE memory, B = n_obstacles / O rows of drcvar_risk_table_fill, 16-byte aligned,
 *          written before the launch on the same stream or earlier, never by it
 *   state: one 16-byte record, 16-byte aligned (read when the kernel runs); out [unit_count, 8];
 *   status [unit_count] or NULL
 *
 * The table is device memory: this entry CANNOT check that it holds B rows or that it was filled
 * for this n_samples.  The caller keeps the table, B and n_samples together (the Python layer
 * does: engine.RiskTable.to_device and engine.prepare_sampled_halfspaces_risk).
 *
 * Host checks: n_obstacles_per_problem < 1, draw_period < 1, n_obstacles not a multiple of
 * n_obstacles_per_problem, a null or misaligned table (when something would be launched), a unit
 * window outside [0, B O T), and everything drcvar_sampled_halfspaces_f64_dev rejects for the
 * arguments the two entries share (a null nominal_path, ego_path, out or state, a state that is
 * not 16-byte aligned, path_steps < 1, ...): DRCVAR_ERR_INVALID_ARGUMENT.  Its limits (n_samples,
 * the grid): DRCVAR_ERR_UNSUPPORTED.  unit_count == 0: DRCVAR_OK, nothing is launched.
 * Asynchronous on `stream`, no allocation, no synchronisation; capturable.
 */
int drcvar_sampled_halfspaces_f64_risk(
    const double* nominal_path, int64_t n_obstacles, int64_t path_steps, int64_t nom_so,
    int64_t nom_st, int64_t n_steps, int64_t unit_begin, int64_t unit_count, int64_t n_samples,
    double l00, double l10, double l11, uint64_t seed, const drcvar_step_state* state,
    int32_t zero_first_step, const double* ego_path, int64_t ego_stride,
    int64_t n_obstacles_per_problem, const void* table, int64_t draw_period, double* out,
    int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRCVAR_LOOP_RISK_H */
