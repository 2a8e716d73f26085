/*
 * drcvar_loop_eval.h — C ABI of the loop-evaluation library (libdrcvar_loop_eval.so): the
 * out-of-sample collision evaluation of receding-horizon loops WHILE they run, built beside the
 * engine library from csrc/drcvar_clearance.hip (compiled once more with DRCVAR_LOOP_EVAL_LIBRARY).
 * The engine library's symbol list (33 symbols, ABI 3) and the loop library's (drcvar_loop.h) are
 * unchanged by it.  Conventions, return codes and drcvar_step_state: drcvar_sampling.h.
 */
#ifndef DRCVAR_LOOP_EVAL_H
#define DRCVAR_LOOP_EVAL_H

#include <stdint.h>

#include "drcvar_sampling.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The device-state, batched, one-row form of drcvar_min_clearance_f64: one launch evaluates the
 * CURRENT state of each of n_problems loops against n_realizations noise realisations of its
 * obstacles, and accumulates into a running minimum and into per-step collision counts.  Issued
 * after drcvar_mpc_step_advance[_batch]_f64 on the same stream (x0 is then the state just reached
 * and state[b].step its path row), it joins a captured control step: nothing per-step is frozen.
 *
 * For problem b = 0 .. n_problems - 1, with s = state[b].step, i = s - step_begin (the wrapped
 * 64-bit difference, as the advance entry forms it) and c(r) = min(max(r, 0), path_steps - 1):
 * problem b is evaluated only when i <= log_rows (as an unsigned number) and 0 <= s < noise_steps;
 * otherwise nothing of problem b is read or written beyond state[b].  When it is evaluated,
 *
 *   ego = c_out x0[b]               each coordinate an fma chain over j = 0 .. n_states - 1 from +0.0
 *   d2(m, o) = |ego - (nominal_path[b * n_obstacles + o, c(s)] + noise(m, o))|^2
 *                                   (px = nom + n, dx = ego - px, fma(dx, dx, dy * dy): the
 *                                   expressions of drcvar_min_clearance_f64)
 *   min_d2[b, m]    = min(min_d2[b, m], min over o of d2(m, o))         m = 0 .. n_realizations - 1
 *   step_hits[b, i] += #{m : min over o of d2(m, o) < combined_radius^2}        (when not NULL)
 *
 * noise(m, o) is bit for bit the draw drcvar_min_clearance_f64 makes for (seed, stream_offset =
 * eval_offset + b * problem_offset_stride mod 2^64, realisation m, obstacle o, step t = s) in a
 * call with n_obstacles obstacles and n_steps = noise_steps: Philox counter
 * g = m * (n_obstacles * noise_steps) + o * noise_steps + s.  With zero_first_step, s = 0 has no
 * noise (no Philox call).  problem_offset_stride = 0: every problem sees the same realisations
 * (common random numbers across loops); 1: independent ones.  noise_kind, p0, p1, p2 and
 * combined_radius are drcvar_min_clearance_f64's.
 *
 * Non-finite positions follow IEEE 754, as in drcvar_min_clearance_f64 (NaN propagates through
 * every minimum; the running one included):
 *   min_d2[b, m] becomes NaN at the first evaluated launch in which some d2(m, o) is NaN, and stays
 *     NaN through every later launch (a NaN the caller stored stays as well).
 *   The launch that met the NaN adds nothing to step_hits[b, i] for that m; every launch counts by
 *     its own d2 alone, so later launches count that m again when their d2 are not NaN.
 *   The other problems keep their bits.  d2 = +inf (one infinite coordinate) is an ordinary member
 *     of the minimum; inf - inf is NaN.
 *
 * The entry ACCUMULATES: the caller sets min_d2 to +inf and step_hits to 0 before the first launch.
 * Exactly one thread owns (b, m) in a launch and launches are ordered by the stream alone; the
 * result does not depend on the launch geometry.  The clearance is sqrt(min_d2) - combined_radius,
 * formed by the caller.
 *
 *   x0 [B, n_states] dense; c_out [2, n_states] row-major HOST memory, copied at call time
 *   nominal_path [B * n_obstacles, path_steps, 2]: obstacle stride nom_so, row stride nom_st
 *                                                  (doubles), adjacent coordinates
 *   state [B] 16-byte records, base 16-byte aligned; only .step is read, nothing is written
 *   min_d2 [B, n_realizations]: row stride out_sb (doubles), adjacent realisations
 *   step_hits [B, log_rows + 1] int64, dense, or NULL      B = n_problems
 *
 * Host checks: a negative n_problems, n_obstacles, n_realizations or noise_steps, a p0, p1 or p2
 * that is NaN or infinite (the noise itself must be finite), a NaN combined_radius,
 * a negative Laplace scale, combined_radius < 0, noise_kind outside {0, 1}, n_states outside 1..8,
 * path_steps < 1, log_rows < 0: DRCVAR_ERR_INVALID_ARGUMENT.  Then n_problems, n_realizations or
 * n_obstacles equal to 0: DRCVAR_OK, nothing is launched and no pointer is looked at.  Then a null
 * x0, c_out, nominal_path, state or min_d2, or a state not 16-byte aligned:
 * DRCVAR_ERR_INVALID_ARGUMENT.  Then n_obstacles * noise_steps > 2^20, n_realizations > 2^40 or a
 * grid dimension over its limit (n_problems > 65535): DRCVAR_ERR_UNSUPPORTED.  noise_steps == 0:
 * DRCVAR_OK, nothing is launched (no step is evaluated).  Asynchronous on `stream`, no allocation,
 * no synchronisation; capturable.
 */
int drcvar_loop_clearance_f64(int64_t n_problems, const double* x0, int32_t n_states,
                              const double* c_out, const double* nominal_path, int64_t n_obstacles,
                              int64_t path_steps, int64_t nom_so, int64_t nom_st,
                              const drcvar_step_state* state, int64_t step_begin, int64_t log_rows,
                              int64_t noise_steps, int32_t noise_kind, double p0, double p1,
                              double p2, double combined_radius, int64_t n_realizations,
                              uint64_t seed, uint64_t eval_offset, uint64_t problem_offset_stride,
                              int32_t zero_first_step, double* min_d2, int64_t out_sb,
                              int64_t* step_hits, void* stream);

/*
 * The same with the launch geometry spelled out: realizations_per_thread = 0 is the entry above
 * (the library's rule), 1 .. 64 makes every thread take that many realisations (a workgroup then
 * covers 256 * realizations_per_thread of them); negative: DRCVAR_ERR_INVALID_ARGUMENT, above 64:
 * DRCVAR_ERR_UNSUPPORTED.  Every setting gives the same bits.
 */
int drcvar_loop_clearance_f64_ex(int64_t n_problems, const double* x0, int32_t n_states,
                                 const double* c_out, const double* nominal_path,
                                 int64_t n_obstacles, int64_t path_steps, int64_t nom_so,
                                 int64_t nom_st, const drcvar_step_state* state, int64_t step_begin,
                                 int64_t log_rows, int64_t noise_steps, int32_t noise_kind,
                                 double p0, double p1, double p2, double combined_radius,
                                 int64_t n_realizations, uint64_t seed, uint64_t eval_offset,
                                 uint64_t problem_offset_stride, int32_t zero_first_step,
                                 double* min_d2, int64_t out_sb, int64_t* step_hits,
                                 int32_t realizations_per_thread, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DRCVAR_LOOP_EVAL_H */
