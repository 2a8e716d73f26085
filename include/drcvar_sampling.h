/*
 * drcvar_sampling.h — C ABI of the MI355X (gfx950) obstacle-sample generator.
 *
 * The reference draws every obstacle's Monte Carlo sample trajectories on the host
 * (simulation/obstacles.py:43-77 generate_obstacle_sample_trajectories: per step, n_samples draws
 * of N(0, noise_cov) added to the nominal position; step 0 noise-free, :63) and the caller ships
 * them to the solver.  This entry point generates the same distribution directly in device memory,
 * in the layout drcvar_safe_halfspaces_f64 consumes, so a GPU pipeline never stages samples
 * through the host.
 *
 *   drcvar_sample_trajectories_f64   replaces simulation/obstacles.py:43-77 (and the per-obstacle
 *                                    loop of generate_obstacle_scenarios, :150-163) for a batch
 *                                    of obstacles.
 *   drcvar_sample_units_f64          the same draws for a contiguous block of (obstacle, step)
 *                                    units of a global batch (one rank's shard).
 *   drcvar_min_clearance_f64[_ex]    Monte Carlo out-of-sample evaluation: many noise realisations
 *                                    of the obstacles drawn by the same generator and reduced to
 *                                    each trajectory's minimum clearance (documented at its
 *                                    declaration below); many-realisation form of main.py:128-138.
 *
 * Random numbers: Philox4x32-10 (counter-based; key = seed, counter = (unit * ceil(N/2) + pair,
 * stream)), one call per PAIR of samples of a unit -> two (32-bit uniform, 32-bit turn) pairs ->
 * Box-Muller -> z ~ N(0, I2); sample = nominal + L z with L the lower Cholesky factor of noise_cov
 * (for L = l I, l > 0 — the reference's default — the kernel folds l^2 into the log of Box-Muller
 * and adds l z directly: the same values to a few ulp).
 * Tail: the radius uniform is 32-bit (u = (2x + 1) 2^-33 >= 2^-33), so |z| <= sqrt(66 ln 2) = 6.76
 * and the far tail is quantised in steps of 2^-32 in u; the reference's 53-bit draws exceed 6.76 sd
 * with probability 2^-33 per sample (~0.0075 samples per 128 M-sample C5 refill).  Below the cap the
 * Rayleigh tail frequencies are kept (tests/test_sampling.py::test_device_sampler_radius_tail).
 * Same distribution as the reference's
 * np.random.multivariate_normal, not the same stream (numpy's MT19937 is sequential; the host
 * mirror in simulation/obstacles.py reproduces that stream exactly).  Output is a pure function
 * of (seed, stream_offset, indices): deterministic and independent of the launch geometry.
 *
 * Conventions as in drcvar_halfspace.h (device pointers, caller-owned buffers, strides in doubles,
 * async on `stream`, DRCVAR_* return codes).
 */
#ifndef DRCVAR_SAMPLING_H
#define DRCVAR_SAMPLING_H

#include <stdint.h>

#include "drcvar_halfspace.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * nominal      [n_obstacles, n_steps, 2] nominal positions (strides nom_so, nom_st; coords adjacent)
 * l00,l10,l11  lower Cholesky factor of the 2x2 noise covariance (reference default diag(0.01, 0.01)
 *              -> 0.1, 0, 0.1; simulation/obstacles.py:134)
 * seed         Philox key; stream_offset selects an independent stream (e.g. per rank)
 * zero_first_step  nonzero: step 0 is the nominal position for every sample (obstacles.py:63)
 * out          [n_obstacles, n_steps, n_samples, 2] with strides (so, st, sn), coords adjacent
 */
int drcvar_sample_trajectories_f64(const double* nominal, int64_t n_obstacles, int64_t n_steps,
                                   int64_t nom_so, int64_t nom_st, int64_t n_samples, double l00,
                                   double l10, double l11, uint64_t seed, uint64_t stream_offset,
                                   int32_t zero_first_step, double* out, int64_t so, int64_t st,
                                   int64_t sn, void* stream);

/*
 * Units [unit_begin, unit_begin + unit_count) of the global [n_obstacles, n_steps] grid (unit
 * u = o * n_steps + t), written flat: unit u at out + (u - unit_begin) * su, sample i at + i * sn.
 * Every sample is the one drcvar_sample_trajectories_f64 draws for the whole grid (same Philox
 * counter u * n_samples + i), so a rank can draw its shard of a global batch without the rest
 * (per-rank sampling of contiguous unit blocks).  nominal is the GLOBAL
 * [n_obstacles, n_steps, 2] path.
 */
int drcvar_sample_units_f64(const double* nominal, int64_t n_obstacles, int64_t n_steps,
                            int64_t nom_so, int64_t nom_st, int64_t unit_begin, int64_t unit_count,
                            int64_t n_samples, double l00, double l10, double l11, uint64_t seed,
                            uint64_t stream_offset, int32_t zero_first_step, double* out,
                            int64_t su, int64_t sn, void* stream);

/*
 * Monte Carlo out-of-sample collision evaluation (csrc/drcvar_clearance.hip).  The reference checks
 * its filtered trajectories against ONE Laplace realisation per obstacle (main.py:128-138,
 * simulation/obstacles.py:79-113, simulation/environment.py:108-140); this entry draws
 * n_realizations of them on the device and reduces each to the trajectory's minimum clearance
 * without storing a realisation.
 *
 * For realisation m in [m_begin, m_begin + n_realizations), obstacle o, step t, trajectory k:
 *   one Philox4x32-10 call per (m, o, t): counter (g lo, g hi, stream_offset lo, hi),
 *   g = m * (O * T) + o * T + t, key = seed (the sampler's convention).  The draw is a pure function
 *   of (seed, stream_offset, m, o, t, O, T): independent of the launch geometry, of K and of the
 *   [m_begin, m_begin + M) window that asks for it.  Words x0..x3, E(x) = -log((x + 1/2) 2^-32):
 *     noise_kind 1 (Laplace, per axis)  n = (p0 (E(x0) - E(x1)), p1 (E(x2) - E(x3))), scales
 *                  bx = p0, by = p1 >= 0, p2 ignored: the reference's scale * (e1 - e2),
 *                  a difference of two Exp(1) draws (obstacles.py:106-108), with
 *                  scale = sqrt(diag(noise_cov) / 2) (:100);
 *     noise_kind 0 (Gaussian N(0, L L^T), L = [[p0, 0], [p1, p2]])  (x0, x1) -> Box-Muller -> z,
 *                  n = L z as in the sampler; x2 and x3 are unused.
 *   zero_first_step nonzero: t = 0 carries no noise and makes no Philox call (obstacles.py:96).
 *   d2(k, m, o, t) = |ego[k, t] - (nominal[o, t] + n(m, o, t))|^2: all K trajectories see the same
 *   draws (common random numbers).
 *
 * ego            [n_traj, n_steps, 2] positions (strides ego_sk, ego_st; coords adjacent)
 * nominal        [n_obstacles, n_steps, 2] (strides nom_so, nom_st; coords adjacent)
 * combined_radius  R = robot radius + obstacle radius
 * min_clearance  [n_traj, n_realizations], row stride out_sk:
 *                min_clearance[k, m - m_begin] = sqrt(min over (o, t) of d2) - R
 *                (one correctly rounded sqrt, taken at the end)
 * step_hits      [n_traj, n_steps] contiguous, or NULL: step_hits[k, t] = #{m : min over o of
 *                d2 < R * R} (R * R rounded once on the host).  The call SETS it.
 * step_splits    (_ex) workgroup rows the step range is split over; 0 = chosen from the sizes.  The
 *                result does not depend on it, bit for bit.
 *
 * 1 <= n_traj <= 8, n_obstacles * n_steps <= 2^20, m_begin + n_realizations <= 2^40 (m_begin = 2^40
 * with n_realizations = 0 included) and n_realizations <= 2^39 - 256 per call (a workgroup takes 256
 * realisations and the grid has at most 2^31 - 1 workgroups), otherwise DRCVAR_ERR_UNSUPPORTED.  A
 * null pointer, a negative size, a negative Laplace scale, a negative radius, or a p0, p1 or p2 that
 * is NaN or infinite (the noise itself must be finite): DRCVAR_ERR_INVALID_ARGUMENT.
 * n_realizations == 0: DRCVAR_OK, no kernel launched.  n_obstacles * n_steps == 0 with
 * n_realizations > 0: min_clearance is filled with +inf.
 *
 * Non-finite positions follow IEEE 754, as the NumPy restatement of these formulas does (NaN
 * propagates through every minimum), and never cause an out-of-range access (no index depends on
 * data):
 *   min_clearance[k, m] is NaN exactly when some d2(k, m, o, t) of the call is NaN.  Every other
 *     element has the bits it has without the NaN: a NaN in trajectory k changes nothing in the rows
 *     k' != k, and a NaN in a nominal position makes NaN every clearance it enters.
 *   step_hits[k, t] counts the m for which min over o of d2 < R * R; a minimum with a NaN member is
 *     NaN and counts nothing.  The counts of the other steps are unchanged.
 *   An infinite coordinate is not a NaN: d2 = +inf is an ordinary member of the minimum (it never
 *     wins against a finite one and never counts as a hit); inf - inf, an ego and an obstacle
 *     coordinate infinite with the same sign, is NaN.
 * This holds for both noise kinds, at the noise-free step 0 as at the others, and for every
 * step_splits.
 */
int drcvar_min_clearance_f64(const double* ego, int64_t n_traj, int64_t ego_sk, int64_t ego_st,
                             const double* nominal, int64_t n_obstacles, int64_t n_steps,
                             int64_t nom_so, int64_t nom_st, int32_t noise_kind, double p0,
                             double p1, double p2, double combined_radius, int64_t m_begin,
                             int64_t n_realizations, uint64_t seed, uint64_t stream_offset,
                             int32_t zero_first_step, double* min_clearance, int64_t out_sk,
                             int64_t* step_hits, void* stream);

int drcvar_min_clearance_f64_ex(const double* ego, int64_t n_traj, int64_t ego_sk, int64_t ego_st,
                                const double* nominal, int64_t n_obstacles, int64_t n_steps,
                                int64_t nom_so, int64_t nom_st, int32_t noise_kind, double p0,
                                double p1, double p2, double combined_radius, int64_t m_begin,
                                int64_t n_realizations, uint64_t seed, uint64_t stream_offset,
                                int32_t zero_first_step, double* min_clearance, int64_t out_sk,
                                int64_t* step_hits, int32_t step_splits, void* stream);

/*
 * Safe halfspaces straight from the nominal paths (csrc/drcvar_sampled.hip): replaces
 * generate_obstacle_sample_trajectories (simulation/obstacles.py:43-77) followed by
 * compute_safe_halfspaces (core/halfspaces.py:196-248) over the horizon loop
 * (simulation/environment.py:82-104) — on the device, drcvar_sample_units_f64 followed by
 * drcvar_safe_halfspaces_f64_v2 — by ONE launch that draws each unit's samples into registers,
 * reduces them to the unit's record and stores nothing else.  No sample buffer is allocated.
 *
 * Units [unit_begin, unit_begin + unit_count) of the global [n_obstacles, n_steps] grid, unit
 * u = o * n_steps + t.  The samples of unit u are bit for bit those drcvar_sample_units_f64 writes
 * for the same (nominal, n_samples, L, seed, stream_offset, zero_first_step): same Philox counter,
 * same pairing, same arithmetic.  The record is that of drcvar_safe_halfspaces_f64_v2 on those
 * samples: the same mathematics (fp64 mean, separating direction, exact order statistic of rank
 * min(floor(alpha N), N - 1), L = tau + dsum / k, the same sentinels and status bits), summed in
 * this kernel's own fixed order, so the two agree to rounding, and each is bitwise reproducible.
 *
 * nominal      [n_obstacles, n_steps, 2] GLOBAL nominal path (strides nom_so, nom_st; coords adjacent)
 * ego          [n_steps, 2] (row stride ego_stride; coords adjacent): the unit's step picks the row
 * out          [unit_count, DRCVAR_OUT_WIDTH] contiguous records, DRCVAR_COL_*
 * status       [unit_count] DRCVAR_UNIT_* bits, or NULL
 * samples_out  NULL, or the kernel also stores the samples it drew: unit u at
 *              samples_out + (u - unit_begin) * su, sample i at + i * sn, coordinates adjacent.
 *              The records are the same bits with and without it.
 *
 * 1 <= n_samples <= DRCVAR_MAX_SAMPLES.  Checked on the host before any launch: a null nominal, ego
 * or out, a negative size, a unit range outside the grid, a NaN factor or a parameter
 * drcvar_safe_halfspaces_f64 rejects: DRCVAR_ERR_INVALID_ARGUMENT; n_samples > DRCVAR_MAX_SAMPLES,
 * a grid beyond the sampler's limits (2^40) or more than 2^31 - 1 units in one call:
 * DRCVAR_ERR_UNSUPPORTED; unit_count == 0 or n_samples == 0: DRCVAR_OK, nothing launched.
 * Unit-level exits (sentinels + status) as in drcvar_safe_halfspaces_f64_v2: alpha N > N,
 * epsilon < 0, a non-finite sum (here from a non-finite nominal position or factor).
 * Asynchronous on `stream`, no allocation, no synchronisation: the call can be captured in a graph
 * (a captured launch replays the same draw; drcvar_sampled_halfspaces_f64_dev below reads the
 * stream offset from device memory instead, for a fresh draw per replay).
 */
int drcvar_sampled_halfspaces_f64(
    const double* nominal, int64_t n_obstacles, int64_t n_steps, int64_t nom_so, int64_t nom_st,
    int64_t unit_begin, int64_t unit_count, int64_t n_samples,
    double l00, double l10, double l11, uint64_t seed, uint64_t stream_offset,
    int32_t zero_first_step,
    const double* ego, int64_t ego_stride,
    double robot_radius, double obstacle_radius, double alpha, double delta, double epsilon,
    double* out, int32_t* status,
    double* samples_out, int64_t su, int64_t sn,
    void* stream);

/* device-resident, 16-byte aligned; read by the kernels at launch time, so a captured launch
 * follows it from replay to replay */
typedef struct drcvar_step_state {
  uint64_t stream_offset;  /* the Philox stream words of this step's draw */
  int64_t  step;           /* first path row of this step's window */
} drcvar_step_state;

/*
 * The device-state form of drcvar_sampled_halfspaces_f64, for a receding-horizon loop replayed
 * from one graph: the window's first path row and the stream offset are read from `state` when the
 * kernel runs, not frozen at the call.
 *
 * nominal_path [n_obstacles, path_steps, 2] (strides nom_so, nom_st) and ego_path [path_steps, 2]
 * (row stride ego_stride) are whole paths; the launch evaluates the window of n_steps = T rows that
 * starts at s = state->step.  With c(i) = min(max(i, 0), path_steps - 1), window unit (o, t),
 * u = o * T + t, uses nominal_path[o, c(s + t)] and ego_path[c(s + t)]: past either end of a path
 * the obstacle and the ego hold the end row, and no value of `state` causes an out-of-range access.
 * The Philox counter is u * ceil(N/2) + pair with the WINDOW-RELATIVE u, the stream words are
 * state->stream_offset, the key is `seed`; zero_first_step applies to the window's t == 0 (the
 * obstacle's current position is known, simulation/obstacles.py:63).
 *
 * The launch writes the same record bytes and status words as drcvar_sampled_halfspaces_f64 called
 * on the gathered window nominal_path[:, c(s .. s+T-1)], ego_path[c(s .. s+T-1)] with
 * stream_offset = state->stream_offset.  There is no samples_out.
 *
 * `state` is read with the kernel's first (scalar) load.  Whatever writes it — an earlier kernel or
 * copy on the same stream, e.g. drcvar_mpc_step_advance_f64 (drcvar_mpc.h) — must precede this
 * launch in stream order; nothing may write it while the launch runs.
 *
 * Host checks: those of drcvar_sampled_halfspaces_f64, and DRCVAR_ERR_INVALID_ARGUMENT for
 * path_steps < 1, n_steps < 0, and (once there is something to launch) a `state` that is null or
 * not 16-byte aligned.  unit_count == 0 or n_samples == 0: DRCVAR_OK, nothing launched.
 */
int drcvar_sampled_halfspaces_f64_dev(
    const double* nominal_path, int64_t n_obstacles, int64_t path_steps, int64_t nom_so, int64_t nom_st,
    int64_t n_steps,            /* window length T: units u = o * T + t, t = 0 .. T-1 */
    int64_t unit_begin, int64_t unit_count, int64_t n_samples,
    double l00, double l10, double l11, uint64_t seed,
    const drcvar_step_state* state, int32_t zero_first_step,
    const double* ego_path, int64_t ego_stride,   /* [path_steps, 2] */
    double robot_radius, double obstacle_radius, double alpha, double delta, double epsilon,
    double* out, int32_t* status, void* stream);

/* host only: the plan a sample count runs on (threads per unit, Philox pairs per thread; a plan
 * holds 2 * threads * pairs samples); DRCVAR_ERR_UNSUPPORTED above DRCVAR_MAX_SAMPLES */
int drcvar_sampled_launch_plan(int64_t n_samples, int32_t* threads, int32_t* pairs_per_thread);

#ifdef __cplusplus
}
#endif

#endif /* DRCVAR_SAMPLING_H */
