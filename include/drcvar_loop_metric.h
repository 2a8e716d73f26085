/*
 * drcvar_loop_metric.h — C ABI of the metric library (libdrcvar_loop_metric.so): the sampled
 * halfspaces of a batch of receding-horizon loops whose METRIC (mean, CVaR or DR-CVaR) is each
 * problem's own, beside its own risk parameters and the draws shared by choice of
 * drcvar_loop_risk.h.  Built beside the engine library from csrc/drcvar_sampled.hip (compiled once
 * more with DRCVAR_LOOP_METRIC_LIBRARY).  The engine library's symbol list (33 symbols, ABI 3), the
 * loop library's (drcvar_loop.h), the loop-evaluation library's (drcvar_loop_eval.h), the
 * predicted-ego library's (drcvar_loop_pred.h) and the risk-table library's (drcvar_loop_risk.h)
 * are unchanged by it.  Conventions, return codes and drcvar_step_state: drcvar_sampling.h.
 */
#ifndef DRCVAR_LOOP_METRIC_H
#define DRCVAR_LOOP_METRIC_H

#include <stdint.h>

#include "drcvar_sampling.h"

#ifdef __cplusplus
extern "C" {
#endif

/* metric[b]: which halfspace of its units' records problem b filters with */
#define DRCVAR_METRIC_MEAN 0
#define DRCVAR_METRIC_CVAR 1
#define DRCVAR_METRIC_DR_CVAR 2

/* columns of a row of `selected` (the fourth double of a row is +0.0) */
#define DRCVAR_SEL_H0 0
#define DRCVAR_SEL_H1 1
#define DRCVAR_SEL_G 2
#define DRCVAR_SEL_WIDTH 4

/*
 * The bytes of a risk-table row as this library reads it.  The rows are those of
 * drcvar_risk_table_fill (drcvar_loop_risk.h), made from the same source, so this equals
 * drcvar_risk_table_row_bytes(); a caller that loads both libraries checks the equality once.
 */
int64_t drcvar_metric_table_row_bytes(void);

/*
 * drcvar_sampled_halfspaces_f64_risk with a metric per problem: the arguments of that entry in
 * their order, and
 *
 *   metric   [B] int32, DEVICE memory, B = n_obstacles / n_obstacles_per_problem: written before
 *            the launch on the same stream or earlier, never by it
 *   selected [unit_count, DRCVAR_SEL_WIDTH] doubles, DEVICE memory
 *
 * Defining property.  The launch writes into `out` and `status` exactly the bytes
 * drcvar_sampled_halfspaces_f64_risk writes for the same arguments.  For the unit in row r of the
 * window (unit unit_begin + r), which belongs to problem b, it also writes
 *
 *   metric[b]                   selected[4 r .. 4 r + 3]
 *   DRCVAR_METRIC_MEAN          (rec[MEAN_H0], rec[MEAN_H1], rec[G_MEAN],     +0.0)
 *   DRCVAR_METRIC_CVAR          (rec[H0],      rec[H1],      rec[G_CVAR],     +0.0)
 *   DRCVAR_METRIC_DR_CVAR       (rec[H0],      rec[H1],      rec[G_DR_TILDE], +0.0)
 *   any other value             (quiet NaN,    quiet NaN,    quiet NaN,       +0.0)
 *
 * where rec = out + 8 r is the unit's record, bit for bit: the lane that stores the record stores
 * the row from the same registers.  With any other code the record and the status word are
 * unaffected and nothing is indexed by the code; a solve on the NaN row fails visibly.  This holds
 * on every exit of the kernel: the normal finish, the non-finite / unbounded exit with its
 * sentinel offsets, and the noise-free first step.
 *
 * `selected` viewed as [B, O, T, 4] gives the solver's hs_h = [..., 0:2] and hs_g = [..., 2] with
 * one stride per dimension and no copy.
 *
 * The entry cannot check device memory: that `metric` holds B codes is the caller's to keep (the
 * Python layer does: engine.prepare_sampled_halfspaces_metric).
 *
 * Host checks: everything drcvar_sampled_halfspaces_f64_risk rejects, with the same code; a null
 * metric or selected when something would be launched: DRCVAR_ERR_INVALID_ARGUMENT.
 * unit_count == 0: DRCVAR_OK, nothing is launched and no pointer is looked at.  Asynchronous on
 * `stream`, no allocation, no synchronisation; capturable.
 */
int drcvar_sampled_halfspaces_f64_metric(
    const double* nominal_path, int64_t n_obstacles, int64_t path_steps, int64_t nom_so,
    int64_t nom_st, int64_t n_steps, int64_t unit_begin, int64_t unit_count, int64_t n_samples,
    double l00, double l10, double l11, uint64_t seed, const drcvar_step_state* state,
    int32_t zero_first_step, const double* ego_path, int64_t ego_stride,
    int64_t n_obstacles_per_problem, const void* table, int64_t draw_period, const int32_t* metric,
    double* out, int32_t* status, double* selected, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRCVAR_LOOP_METRIC_H */
