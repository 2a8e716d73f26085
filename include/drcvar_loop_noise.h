/*
 * drcvar_loop_noise.h — C ABI of the noise library (libdrcvar_loop_noise.so): a batch of
 * receding-horizon loops whose NOISE FACTOR is each obstacle's and each look-ahead step's own,
 * beside each problem's own route, metric, risk parameters and draws shared by choice
 * (drcvar_loop_route.h, drcvar_loop_metric.h, drcvar_loop_risk.h).  Three entries: the row size of
 * the noise table, its host-side fill, and the sampled halfspaces that read it.  Built beside the
 * engine library from csrc/drcvar_sampled.hip (compiled once more with DRCVAR_LOOP_NOISE_LIBRARY,
 * linked alone).  The engine library's symbol list (33 symbols, ABI 3) and those of the loop,
 * loop-evaluation, predicted-ego, risk-table, metric and route libraries are unchanged by it.
 * Conventions, return codes and drcvar_step_state: drcvar_sampling.h, drcvar_mpc.h.
 */
#ifndef DRCVAR_LOOP_NOISE_H
#define DRCVAR_LOOP_NOISE_H

#include <stdint.h>

#include "drcvar_sampling.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The noise table: [noise_period * T] rows of drcvar_noise_table_row_bytes() bytes each (a
 * multiple of 16), T the launch's n_steps, in device memory at a 16-byte aligned address.  With o
 * the launch's global obstacle index in [0, n_obstacles) and t the window-relative step, unit
 * (o, t) reads row (o mod noise_period) * T + t: noise_period 1 is one look-ahead schedule for
 * every obstacle, n_obstacles_per_problem one per obstacle shared by the problems, n_obstacles one
 * per problem and obstacle.  The row layout is private to the library: fill rows on the host with
 * drcvar_noise_table_fill and copy them.
 */
int64_t drcvar_noise_table_row_bytes(void);

/*
 * Host only: fills `rows` rows at `out` (host memory, out_bytes bytes) from chol [rows, 3], the
 * lower Cholesky factors (l00, l10, l11) of the rows' covariances.  A row holds what the host of
 * drcvar_sampled_halfspaces_f64_route would have passed to its kernel for that factor: the three
 * entries, whether the factor takes the sampler's isotropic form (l10 == 0, l00 == l11 > 0,
 * finite, 2^-200 <= l00^2 <= 2^200: the one expression every entry uses) and the log scale of
 * l00^2 in that form, of 1 otherwise.  Equal factors give equal bytes.  Zero, singular and
 * infinite factors are accepted, as that entry accepts them.
 *
 * rows < 0 or out_bytes < 0: DRCVAR_ERR_INVALID_ARGUMENT; rows == 0: DRCVAR_OK, no pointer is
 * looked at; a null pointer, out_bytes below rows * row_bytes or a NaN anywhere in chol:
 * DRCVAR_ERR_INVALID_ARGUMENT, and nothing is written.
 */
int drcvar_noise_table_fill(const double* chol, int64_t rows, void* out, int64_t out_bytes);

/*
 * drcvar_sampled_halfspaces_f64_route (drcvar_loop_route.h) with a noise factor per unit: the
 * arguments of that entry in their order, with l00, l10, l11 replaced by
 *
 *   noise          the noise table (above), noise_period * n_steps rows
 *   noise_period   1 <= noise_period <= n_obstacles
 *
 * The caller keeps noise readable for noise_period * n_steps rows; it is written before the launch
 * on the same stream or earlier, never by it.  zero_first_step makes window step 0 noise-free
 * whatever its row holds.
 *
 * Defining property.  For every unit (o, t) of the launch, its rows of `out`, `status` and
 * `selected` hold the bytes drcvar_sampled_halfspaces_f64_route writes for that unit when called
 * with (l00, l10, l11) equal to the factor of the unit's row and every other argument equal.  A
 * table whose rows are all equal is the route launch, byte for byte.
 *
 * Host checks: noise_period < 1 or above n_obstacles: DRCVAR_ERR_INVALID_ARGUMENT; once there is
 * something to launch (unit_count > 0 and n_samples > 0), noise null or not 16-byte aligned:
 * DRCVAR_ERR_INVALID_ARGUMENT; then everything drcvar_sampled_halfspaces_f64_route rejects, with
 * the same code and in its order.  unit_count == 0: DRCVAR_OK, nothing is launched and no pointer
 * is looked at.  Asynchronous on `stream`, no allocation, no synchronisation; capturable.
 */
int drcvar_sampled_halfspaces_f64_noise(
    const double* nominal_path, int64_t n_obstacles, int64_t path_steps, int64_t nom_so,
    int64_t nom_st, int64_t n_steps, int64_t unit_begin, int64_t unit_count, int64_t n_samples,
    const void* noise, int64_t noise_period, uint64_t seed, const drcvar_step_state* state,
    int32_t zero_first_step, const double* ego_path, int64_t ego_stride,
    int64_t ego_problem_stride, int64_t n_obstacles_per_problem, const void* table,
    int64_t draw_period, const int32_t* metric, double* out, int32_t* status, double* selected,
    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRCVAR_LOOP_NOISE_H */
