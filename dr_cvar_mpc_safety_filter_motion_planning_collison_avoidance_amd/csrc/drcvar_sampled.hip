// drcvar_sampled.hip — safe halfspaces straight from the nominal paths, for gfx950: the unit's
// samples are drawn in the kernel, reduced to its 64-byte record and never stored.
//
// Reference: simulation/obstacles.py:43-77 (generate_obstacle_sample_trajectories) followed by
// core/halfspaces.py:196-248 (compute_safe_halfspaces) over the horizon loop of
// simulation/environment.py:82-104.  On the device that was two launches with an [O, T, N, 2]
// buffer between them (drcvar_sample_trajectories_f64 -> drcvar_safe_halfspaces_f64); here it is
// one launch and no buffer.  One workgroup per unit u = o T + t:
//
//   draw    thread `tid` draws the Philox pairs p = tid + j BLOCK (j < PP) of the unit and keeps
//           both samples of each — (p, p + P), P = ceil(N/2) — in registers: bit for bit the
//           samples drcvar_sample_units_f64 writes (same counter u P + p, stream words and key, the
//           same draw_pair arithmetic, the isotropic LogScale form exactly when the sampler takes
//           it).  The noise-free step 0 makes no Philox call.                    [barrier 0: tables]
//   mean    fp64 sums over all samples in a fixed order                         [barrier 1]
//   h       (mu - ego) / |mu - ego| ([1, 0] below 1e-10), d_i = fma(h0, x_i, h1 y_i)
//   window  the distribution is known, so the histogram window is placed from it:
//           sd_d^2 = (l00 h0 + l10 h1)^2 + (l11 h1)^2 about the unit's own mu_d — no pilot, no
//           moment reduction on the chain to the first barrier               [barriers 2, 3]
//   tau     exact order statistic of rank m = min(floor(alpha N), N - 1): the target bucket's
//           <= 128 candidates ranked directly.  A target outside the window, a crowded bucket or
//           a window that cannot be placed (sd_d not positive or not finite) takes the exact
//           fallback over the register-held d (min/max, value-linear then order-preserving-key
//           histogram refinement, lo == hi exit): nothing is re-read and nothing drawn again.
//   record  L = tau + dsum / k and the offsets, sentinels and status bits of the stored form.
//
// samples_out (optional): the kernel also stores the samples it drew; the record is the same bits.
//
// Seven entries, one kernel template: drcvar_sampled_halfspaces_f64 freezes the stream offset and
// the window in its arguments; drcvar_sampled_halfspaces_f64_dev (DEV below) reads the offset and
// the window's first path row from a 16-byte state in device memory, so that a receding-horizon
// loop can be replayed from one graph with a fresh draw per step (simulation/closed_loop.py);
// drcvar_sampled_halfspaces_f64_pred (PRED below) is the device-state form whose ego is each
// problem's own predicted path; drcvar_sampled_halfspaces_f64_risk (RISK below) is the device-state
// form whose risk parameters are each problem's own row of a table in device memory;
// drcvar_sampled_halfspaces_f64_metric (METRIC below) is the risk-table form that also stores each
// unit's halfspace under its problem's own metric; drcvar_sampled_halfspaces_f64_route (ROUTE
// below) is the metric form whose ego path is each problem's own;
// drcvar_sampled_halfspaces_f64_noise (NOISE below) is the route form whose noise factor is each
// unit's own row of a table in device memory.  The source is compiled six times: into the engine library with the first two entries, with DRCVAR_LOOP_PRED_LIBRARY into a library of its
// own (include/drcvar_loop_pred.h) that holds the third and instantiates only the PRED kernels,
// with DRCVAR_LOOP_RISK_LIBRARY into another (include/drcvar_loop_risk.h) that holds the fourth and
// instantiates only the RISK kernels, and with DRCVAR_LOOP_METRIC_LIBRARY into a last one
// (include/drcvar_loop_metric.h) that holds the fifth and instantiates only the METRIC kernels,
// and with DRCVAR_LOOP_ROUTE_LIBRARY as one of the two objects of the route library
// (include/drcvar_loop_route.h), which holds the sixth and instantiates only the ROUTE kernels,
// and with DRCVAR_LOOP_NOISE_LIBRARY into the noise library (include/drcvar_loop_noise.h), which
// holds the seventh and instantiates only the NOISE kernels.
//
// The draw is the sampler's (drcvar_generator.inc) and the selection the stored form's
// (drcvar_selection.inc); the direction alone differs on purpose, by one more Newton step of the
// reciprocal square root (rsqrt_nr2).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "drcvar_sampling.h"
#ifdef DRCVAR_LOOP_PRED_LIBRARY
#include "drcvar_loop_pred.h"
#endif
#ifdef DRCVAR_LOOP_RISK_LIBRARY
#include "drcvar_loop_risk.h"
#endif
#ifdef DRCVAR_LOOP_ROUTE_LIBRARY
#include "drcvar_loop_route.h"
#endif
#ifdef DRCVAR_LOOP_NOISE_LIBRARY
#include "drcvar_loop_noise.h"
#endif
#include "drcvar_loop_metric.h"  // every build: the METRIC form's constants (no code without it)

namespace {

#include "drcvar_generator.inc"  // the draw: Philox, Box-Muller, the LDS tables, draw_pair
#include "drcvar_selection.inc"  // Params and the selection toolkit of the stored form

// The draw's launch-uniform arguments (the sampler's SampleArgs, without its output).
struct DrawArgs {
  int64_t T, nom_so, nom_st, ego_st, u0, su, sn;
  int n;
  int zero_first;
  double l00, l10, l11;
  PhiloxUniform pu;
  LogScale lg;
};

// The whole record by one lane, plain stores; hands back the mean halfspace it stored.
__device__ __forceinline__ void store_record_mean(double* rec, double mux, double muy, double rc,
                                                  double h0, double h1, const Offsets& g,
                                                  double* m0, double* m1, double* gm) {
  mean_halfspace(mux, muy, rc, m0, m1, gm);
  rec[DRCVAR_COL_MEAN_H0] = *m0;
  rec[DRCVAR_COL_MEAN_H1] = *m1;
  rec[DRCVAR_COL_G_MEAN] = *gm;
  rec[DRCVAR_COL_H0] = h0;
  rec[DRCVAR_COL_H1] = h1;
  rec[DRCVAR_COL_G_CVAR] = g.g_cvar;
  rec[DRCVAR_COL_G_DR_STAR] = g.g_star;
  rec[DRCVAR_COL_G_DR_TILDE] = g.g_tilde;
}

__device__ __forceinline__ void store_record(double* rec, double mux, double muy, double rc,
                                             double h0, double h1, const Offsets& g) {
  double m0, m1, gm;
  store_record_mean(rec, mux, muy, rc, h0, h1, g, &m0, &m1, &gm);
}

// store_record, and by the same lane the unit's halfspace under metric `code` from the values it
// has just stored (core/mpc_filter.METRIC_COLUMNS): sel = (h0, h1, g, +0.0), three quiet NaNs for
// any other code.  Nothing is indexed by the code.
__device__ __forceinline__ void store_record_selected(double* rec, double* sel, int32_t code,
                                                      double mux, double muy, double rc, double h0,
                                                      double h1, const Offsets& g) {
  double m0, m1, gm;
  store_record_mean(rec, mux, muy, rc, h0, h1, g, &m0, &m1, &gm);
  const bool mean = code == DRCVAR_METRIC_MEAN;
  const bool known = mean || code == DRCVAR_METRIC_CVAR || code == DRCVAR_METRIC_DR_CVAR;
  const double nan = __builtin_nan("");
  sel[DRCVAR_SEL_H0] = known ? (mean ? m0 : h0) : nan;
  sel[DRCVAR_SEL_H1] = known ? (mean ? m1 : h1) : nan;
  sel[DRCVAR_SEL_G] = known ? (mean ? gm : (code == DRCVAR_METRIC_CVAR ? g.g_cvar : g.g_tilde)) : nan;
  sel[DRCVAR_SEL_WIDTH - 1] = 0.0;
}

// ---------------------------------------------------------------------------------------------
// the kernel
//   BLOCK    threads per unit (one workgroup per unit)
//   PP       Philox pairs per thread (N <= 2 BLOCK PP)
//   LOG_NB   log2 of the histogram bins
//   ISO      the sampler's isotropic LogScale form
//   DEV      the device-state form (below)
//   PRED     the device-state form with a predicted ego (below; implies DEV)
//   RISK     the device-state form with a risk table (below; implies DEV, never with PRED)
//   METRIC   the risk-table form with a metric per problem (below; implies RISK)
//   ROUTE    the metric form with an ego path per problem (below; implies METRIC)
//   NOISE    the route form with a noise factor per unit (below; implies ROUTE; ISO is unused)
// Blocks of 512 threads are held to 128 VGPRs (four waves per SIMD): two workgroups share a CU,
// so one unit's draw (VALU) overlaps the other's selection (barriers, LDS, one ranking wave).
//
// The device-state form (DEV, drcvar_sampled_halfspaces_f64_dev): the stream words and the
// window's first path row come from `dev.state` in device memory, so a captured launch follows
// them from replay to replay.  Window unit (o, t) takes path row c(step + t), c = clamp to
// [0, path_last]; the Philox counter stays window-relative, so the launch is the base form on the
// gathered window.  One template, one body: without DEV it compiles to the instructions the
// kernel had before the flag existed (hipcc -S, every plan, both ISO forms).
//
// `state` is one uniform 16-byte load (both words of a const __restrict__ kernel argument, read
// before any store: scalar memory).  Its writer is an earlier kernel or copy on the same stream
// (the advance kernel's plain vector stores, drcvar_step.hip): a kernel's stores are written back
// to L2 when it ends, and the scalar and vector L1 caches are invalidated before the next dispatch
// of the in-order queue starts, so the scalar load reads L2's value.  Nothing inside one launch
// writes `state`, so no finer ordering is needed.  PhiloxUniform is then made here, in scalar code
// (one 32 x 32 -> 64 product, three xors), by the make_philox_uniform the host uses; a.pu arrives
// with the key.
//
// The predicted-ego form (PRED, drcvar_sampled_halfspaces_f64_pred): the launch covers B problems
// of O obstacles each, unit u = (b O + o) T + t, and the ego of a unit is its own problem's:
// xs = x0[b] at t = 0, else pred[b, min(t + shift, pred_last)], ego = c_out xs (an fma chain over
// the states from +0.0, as drcvar_loop_clearance_f64 forms it).  Everything else is DEV's, so the
// launch is the base form on the gathered window with that ego.  b = (u / T) / O is uniform over
// the workgroup: x0 and pred are uniform loads of const __restrict__ arguments, written by earlier
// launches on the same stream (the solver, the advance kernel) and never by this one: the
// visibility argument is `state`'s.  The row is clamped to [0, pred_last] for every t and shift;
// b < B is the host's check of the unit window against B O T.  The ego is formed here, before
// barrier 0 and blocks away from the direction's mu - ego: next to it the compiler contracted that
// subtraction differently from the other forms (an ulp of h in 3 units of 24, seen by the bitwise
// tests).  Measured and not kept: the row as one vector load per wave with
// readlane in place of the nx scalar loads, 0.322 -> 0.336 ms per launch at B = 1024, N = 20.
//
// The risk-table form (RISK, drcvar_sampled_halfspaces_f64_risk): the launch covers B problems of
// O obstacles each, unit u = (b O + o) T + t, and the unit's Params are row b of `table` in device
// memory instead of the launch-uniform kernel argument: alpha, delta and epsilon differ from
// problem to problem inside one launch (the rank of the order statistic, 1 / k, the histogram
// window and both unbounded exits with them).  A row is what the host would have passed
// (drcvar_risk_table_fill: make_params with the plan's hist_scale), so per problem the launch is
// the base form with that row's scalars.  b = (u / T) / O is uniform over the workgroup and every
// use of prm was already workgroup-uniform, the early return included: the row is a uniform load
// of a const __restrict__ argument (scalar memory: four s_load of the words the body uses), written
// before the launch and never by it: the visibility argument is `state`'s.  b < B is the host's check of the unit window
// against B O T.  The Philox counter is formed from the draw unit ((b mod D) O + o) T + t in place
// of u: D >= B is DEV's numbering, D = 1 gives every problem the draws of problem 0, and B = S D
// settings-major gives S settings the same D replicate draws (common random numbers).
//
// The metric form (METRIC, drcvar_sampled_halfspaces_f64_metric): the risk-table form, whose lane
// that stores the unit's record also stores selected[row] = (h0, h1, g, +0.0), the halfspace under
// metric[b] (0 mean, 1 CVaR, 2 DR-CVaR; any other code: three quiet NaNs), from the values it holds
// for the record: no launch and no pass over the record is added for a batch whose problems filter
// under different metrics.  out and status are the RISK form's bytes.  metric[b] is one more
// uniform load of a const __restrict__ argument beside the table row, before barrier 0, written
// before the launch and never by it (`state`'s visibility argument); both storing exits (the
// bad / unbounded return and the finish, which the noise-free step reaches too) store the row.
//
// The route form (ROUTE, drcvar_sampled_halfspaces_f64_route): the metric form, whose ego row is
// its own problem's: ego + b ego_ps + r ego_st, with the b the risk-table branch already forms.
// The address stays uniform over the workgroup, so the two coordinates are still scalar loads of a
// const __restrict__ argument written before the launch; one scalar multiply-add is all the form
// adds.  ego_ps = 0 is the metric form's address.
//
// The noise form (NOISE, drcvar_sampled_halfspaces_f64_noise): the route form, whose Cholesky
// factor, isotropic flag and LogScale are row (o mod NP) T + t of `noise` in device memory instead
// of the launch-uniform a.l00, a.l10, a.l11 and a.lg: the assumed covariance differs from obstacle
// to obstacle and from window step to window step inside one launch.  A row is what the host of
// the route entry would have passed for that factor (drcvar_noise_table_fill: the same isotropic
// test, make_log_scale), so per unit the launch is the route form with that row's scalars.  The
// row's address is uniform over the workgroup and the factor entered only in workgroup-uniform
// places (draw_pair's operands, the LDS log table's lam, the window's s0, s1): the row is a
// uniform load of a const __restrict__ argument (scalar memory), before barrier 0 beside the risk
// row and the metric code, written before the launch and never by it: the visibility argument is
// `state`'s.  The LogScale reaches fma_sc and fma_vs in the SGPRs it was loaded into.  Which of
// draw_pair's two forms a unit takes is the row's flag, one uniform branch per Philox call; the
// template's ISO is not read (the library instantiates ISO = false alone).  The host checks
// NP <= n_obstacles; the caller keeps NP T rows readable.
// ---------------------------------------------------------------------------------------------
constexpr int kMaxStates = 8;  // DRCVAR_MPC_MAX_STATES
struct NoState {};
struct DevState {
  const drcvar_step_state* __restrict__ state;
  int64_t path_last;
};
struct PredState {
  const drcvar_step_state* __restrict__ state;
  int64_t path_last;
  const double* __restrict__ x0;    // [B, nx]
  const double* __restrict__ pred;  // [B, pred_last + 1, nx]
  int64_t O, pred_last;             // obstacles per problem; the last row of pred
  int nx, shift;
  double cx[kMaxStates], cy[kMaxStates];  // c_out's two rows, zero past nx
};
struct alignas(16) RiskRow {  // one row of the risk table: Params padded to a multiple of 16 bytes
  Params p;
};
struct RiskState {
  const drcvar_step_state* __restrict__ state;
  int64_t path_last;
  const RiskRow* __restrict__ table;  // [B]
  int64_t O, D;                       // obstacles per problem; the draw period
};
struct MetricState {  // RiskState and the two pointers of the metric form
  const drcvar_step_state* __restrict__ state;
  int64_t path_last;
  const RiskRow* __restrict__ table;
  int64_t O, D;
  const int32_t* __restrict__ metric;  // [B]
  double* __restrict__ selected;       // [units, 4]
};
struct RouteState {  // MetricState and the ego path's stride from problem to problem
  const drcvar_step_state* __restrict__ state;
  int64_t path_last;
  const RiskRow* __restrict__ table;
  int64_t O, D;
  const int32_t* __restrict__ metric;
  double* __restrict__ selected;
  int64_t ego_ps;  // in doubles
};
struct alignas(16) NoiseRow {  // one row of the noise table: a factor as the host would pass it
  double l00, l10, l11;
  int64_t iso;  // 1: the isotropic LogScale form (lg carries l00^2), 0: the general form (lg of 1)
  LogScale lg;
};
struct NoiseState {  // RouteState and the noise table
  const drcvar_step_state* __restrict__ state;
  int64_t path_last;
  const RiskRow* __restrict__ table;
  int64_t O, D;
  const int32_t* __restrict__ metric;
  double* __restrict__ selected;
  int64_t ego_ps;
  const NoiseRow* __restrict__ noise;  // [NP T]
  int64_t NP;                          // the noise period, in obstacles
};

template <int BLOCK, int PP, int LOG_NB, bool ISO, bool DEV = false, bool PRED = false,
          bool RISK = false, bool METRIC = false, bool ROUTE = false, bool NOISE = false>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(BLOCK >= 512 ? 4 : 1)))
sampled_halfspace_kernel(const double* __restrict__ nominal, const double* __restrict__ ego,
                         DrawArgs a, Params prm, double* __restrict__ out,
                         int32_t* __restrict__ status, double* __restrict__ samples_out,
                         std::conditional_t<
                             NOISE, NoiseState,
                             std::conditional_t<
                                 ROUTE, RouteState,
                                 std::conditional_t<
                                     METRIC, MetricState,
                                     std::conditional_t<
                                         RISK, RiskState,
                                         std::conditional_t<
                                             PRED, PredState,
                                             std::conditional_t<DEV, DevState, NoState>>>>>> dev) {
  static_assert(DEV || !PRED, "the predicted-ego form is a device-state form");
  static_assert((DEV && !PRED) || !RISK, "the risk-table form is a device-state form without PRED");
  static_assert(RISK || !METRIC, "the metric form is a risk-table form");
  static_assert(METRIC || !ROUTE, "the route form is a metric form");
  static_assert(ROUTE || !NOISE, "the noise form is a route form");
  constexpr int NW = BLOCK / kWave;
  constexpr int NB = 1 << LOG_NB;
  constexpr int Q = 2 * PP;  // sample slots per thread: 2 j the pair's first, 2 j + 1 its second
  __shared__ double s_turn[kTurnLen], s_log[2 * kLogIdx];
  __shared__ uint32_t hist[hist_words<NB>()];
  __shared__ double cand[NW * kCap];
  __shared__ uint32_t wcount[NW];
  __shared__ uint32_t wbelow_sh[NW];
  __shared__ double red_mom[2 * NW];
  __shared__ double red_rng[2 * NW];
  __shared__ double red_tail[NW];

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid / kWave;
  const int wave_first = __builtin_amdgcn_readfirstlane(tid);  // this wave's first thread: uniform
  const int64_t row = blockIdx.x;                              // the unit's row of out / status
  const int64_t u = a.u0 + row;
  const int64_t o = u / a.T, t = u - o * a.T;
  int64_t ud = u;  // the unit whose Philox counters are drawn
  [[maybe_unused]] int32_t code = 0;  // METRIC: the problem's metric
  [[maybe_unused]] int64_t ego_first = 0;  // ROUTE: where the problem's ego path starts
  if constexpr (RISK) {
    const int64_t b = o / dev.O;
    prm = dev.table[b].p;
    if constexpr (METRIC) code = dev.metric[b];
    if constexpr (ROUTE) ego_first = b * dev.ego_ps;
    ud = ((b % dev.D) * dev.O + (o - b * dev.O)) * a.T + t;
  }
  [[maybe_unused]] bool iso = ISO;  // NOISE: the row's flag
  if constexpr (NOISE) {
    const NoiseRow& nr = dev.noise[(o % dev.NP) * a.T + t];
    a.l00 = nr.l00;
    a.l10 = nr.l10;
    a.l11 = nr.l11;
    a.lg = nr.lg;
    iso = nr.iso != 0;
  }
  int64_t r = t;  // the unit's row of nominal[o] and of ego
  if constexpr (DEV) {
    const uint64_t words = dev.state->stream_offset;
    const int64_t step = dev.state->step;
    a.pu = make_philox_uniform(static_cast<uint32_t>(words), static_cast<uint32_t>(words >> 32),
                               a.pu.k0, a.pu.k1);
    // each word pinned as one scalar value: seen through, the xors that made them are
    // re-associated into the rounds' per-lane xors (two more v_xor per Philox call)
    a.pu.a1 = __builtin_amdgcn_readfirstlane(a.pu.a1);
    a.pu.b1 = __builtin_amdgcn_readfirstlane(a.pu.b1);
    a.pu.c1 = __builtin_amdgcn_readfirstlane(a.pu.c1);
    a.pu.b2 = __builtin_amdgcn_readfirstlane(a.pu.b2);
    // any step: held to [-T, path_last] first, so step + t cannot overflow and clamps the same
    const int64_t s = step < -a.T ? -a.T : (step > dev.path_last ? dev.path_last : step);
    r = s + t < 0 ? 0 : (s + t > dev.path_last ? dev.path_last : s + t);
  }
  const double* nom = nominal + o * a.nom_so + r * a.nom_st;
  const double nx = nom[0], ny = nom[1];
  double e0, e1;
  if constexpr (PRED) {
    const int64_t b = o / dev.O;
    const int64_t pr = t + dev.shift > dev.pred_last ? dev.pred_last : t + dev.shift;
    const double* xs = (t == 0 ? dev.x0 + b * dev.nx
                               : dev.pred + (b * (dev.pred_last + 1) + pr) * dev.nx);
    e0 = e1 = 0.0;
#pragma unroll
    for (int j = 0; j < kMaxStates; ++j) {
      if (j < dev.nx) {
        const double xj = xs[j];
        e0 = fma(dev.cx[j], xj, e0);
        e1 = fma(dev.cy[j], xj, e1);
      }
    }
  } else {
    const double* ep = ego + r * a.ego_st;
    if constexpr (ROUTE) ep = ego + ego_first + r * a.ego_st;
    e0 = ep[0];
    e1 = ep[1];
  }
  const int n = a.n;
  const int pairs = (n + 1) >> 1;  // Philox calls per unit
  const bool noisy = !(a.zero_first && t == 0);  // uniform: the noise-free first step draws nothing
  double* rec = out + row * DRCVAR_OUT_WIDTH;

  if (noisy) load_generator_tables(s_turn, s_log, BLOCK, a.lg.lam);
  for (int b = tid; b < hist_words<NB>(); b += BLOCK) hist[b] = 0u;
  __syncthreads();                                                        // [barrier 0]

  // ---- 1. draw -----------------------------------------------------------------------------
  double x[Q], y[Q];
  uint32_t vmask = 0;  // bit q: slot q holds a sample of the unit
  const uint64_t g0 = static_cast<uint64_t>(ud) * static_cast<uint64_t>(pairs) + static_cast<uint64_t>(tid);
#pragma unroll
  for (int j = 0; j < PP; ++j) {
    const int p = tid + j * BLOCK;
    if (p < pairs) vmask |= 1u << (2 * j);
    if (p + pairs < n) vmask |= 2u << (2 * j);
    x[2 * j] = x[2 * j + 1] = nx;
    y[2 * j] = y[2 * j + 1] = ny;
    // a whole wave past the unit's pairs skips the call; idle lanes of a partly filled wave make
    // it on a counter of their own and drop the result
    if (noisy && wave_first + j * BLOCK < pairs) {
      if constexpr (NOISE) {  // the row's form: uniform over the workgroup
        if (iso)
          draw_pair<true>(g0 + static_cast<uint64_t>(j * BLOCK), a, nx, ny, s_turn, s_log,
                          &x[2 * j], &y[2 * j], &x[2 * j + 1], &y[2 * j + 1]);
        else
          draw_pair<false>(g0 + static_cast<uint64_t>(j * BLOCK), a, nx, ny, s_turn, s_log,
                           &x[2 * j], &y[2 * j], &x[2 * j + 1], &y[2 * j + 1]);
      } else {
        draw_pair<ISO>(g0 + static_cast<uint64_t>(j * BLOCK), a, nx, ny, s_turn, s_log, &x[2 * j],
                       &y[2 * j], &x[2 * j + 1], &y[2 * j + 1]);
      }
    }
  }
  if (samples_out) {  // unit row `row`, sample i at + i sn, coordinates adjacent
    double* dst = samples_out + row * a.su;
#pragma unroll
    for (int j = 0; j < PP; ++j) {
      const int64_t i0 = tid + j * BLOCK, i1 = i0 + pairs;
      if ((vmask >> (2 * j)) & 1u) {
        dst[i0 * a.sn] = x[2 * j];
        dst[i0 * a.sn + 1] = y[2 * j];
      }
      if ((vmask >> (2 * j + 1)) & 1u) {
        dst[i1 * a.sn] = x[2 * j + 1];
        dst[i1 * a.sn + 1] = y[2 * j + 1];
      }
    }
  }

  // ---- 2. mean (fp64, fixed order) and direction ---------------------------------------------
  double sx = 0.0, sy = 0.0;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const bool valid = (vmask >> q) & 1u;
    sx += valid ? x[q] : 0.0;
    sy += valid ? y[q] : 0.0;
  }
  sx = wave_reduce<OpAdd>(sx);
  sy = wave_reduce<OpAdd>(sy);
  if constexpr (NW > 1) {
    if (lane == 0) {
      red_mom[wave] = sx;
      red_mom[NW + wave] = sy;
    }
    __syncthreads();                                                      // [barrier 1]
    sx = sum_partials<NW>(red_mom);
    sy = sum_partials<NW>(red_mom + NW);
  }
  const double mux = sx * prm.inv_n, muy = sy * prm.inv_n;
  // a non-finite nominal position or factor makes a sum non-finite: solver failure
  const bool bad = !(std::isfinite(sx) && std::isfinite(sy));
  double h0, h1;
  separating_direction<rsqrt_nr2>(mux, muy, e0, e1, prm.degenerate_sq, &h0, &h1);
  if (bad || prm.unbounded) {  // risk_metrics.py:298-303,334-338
    if (tid == 0) {
      const double r = prm.rc * norm_h(h0, h1);
      if constexpr (METRIC)
        store_record_selected(rec, dev.selected + row * DRCVAR_SEL_WIDTH, code, mux, muy, prm.rc,
                              h0, h1, failure_offsets(r));
      else
        store_record(rec, mux, muy, prm.rc, h0, h1, failure_offsets(r));
      if (status) status[row] = failure_status(bad, prm);
    }
    return;  // uniform across the workgroup
  }

  // ---- 3. projections; window from the known distribution -------------------------------------
  double d[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q)  // +inf padding: never below, inside or a candidate
    d[q] = ((vmask >> q) & 1u) ? project(h0, h1, x[q], y[q]) : INFINITY;
  const double mu_d = h0 * mux + h1 * muy;
  // h^T L = (l00 h0 + l10 h1, l11 h1): the projection's variance under N(nominal, L L^T)
  const double s0 = fma(a.l00, h0, a.l10 * h1), s1 = a.l11 * h1;
  const double var_d = fma(s0, s0, s1 * s1);
  const double inv_sd = rsqrt_nr(var_d);
  const double sd_d = var_d * inv_sd;
  const double wlo = fma(prm.z_lo, sd_d, mu_d);
  const double scale = prm.hist_scale * inv_sd;
  const LinearMap map{scale, -wlo * scale};
  const uint32_t rank = prm.rank;
  // any positive scale keeps the map monotone: an ill-placed window costs the fallback, never
  // exactness
  bool fast = noisy && var_d > 0.0 && std::isfinite(map.scale) && std::isfinite(map.off) &&
              map.scale > 0.0;
  constexpr double kNB = static_cast<double>(NB);
  uint32_t rr = rank, c = 0;
  int bin = 0;
  double sq = 0.0;  // sum over samples below the target bucket of (d - mu_d)
  if (fast) {
    uint32_t wbelow = 0;  // samples of this wave below the window (wave-uniform)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const double tv = map(d[q]);
      const bool low = tv < 0.0;
      wbelow += static_cast<uint32_t>(__popcll(__ballot(low)));
      sq += low ? d[q] - mu_d : 0.0;
      if (!low && tv < kNB) atomicAdd(&hist[hist_slot<NB>(static_cast<int>(tv))], 1u);
    }
    if (lane == 0) wbelow_sh[wave] = wbelow;
    __syncthreads();                                                      // [barrier 2]
    uint32_t below = 0;  // all samples below the window
#pragma unroll
    for (int w = 0; w < NW; ++w) below += wbelow_sh[w];
    if (rank >= below) {
      const ScanResult sr = scan_bins<NB>(hist, rank - below, lane);  // every wave, same result
      bin = sr.bin;
      rr = rank - below - sr.below;
      c = sr.cnt;
      fast = sr.found && c <= kCap;  // tau above the window, or a crowded bucket: fallback
    } else {
      fast = false;                  // tau below the window: fallback
    }
  }

  // ---- 4. candidates of the target bucket + tail sum below them ------------------------------
  double tau, dsum;  // dsum = sum_{d<tau} (d - tau)
  if (fast) {
    uint32_t wbase = 0;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      // the bucket again, from the same fma: the same bin the histogram counted
      const double tv = map(d[q]);
      const bool inw = !(tv < 0.0) && tv < kNB;
      const int b = inw ? static_cast<int>(tv) : NB;
      sq += b < bin ? d[q] - mu_d : 0.0;
      append_candidate(cand + wave * kCap, wbase, b == bin, d[q], lt_mask);
    }
    sq = wave_reduce<OpAdd>(sq);
    if (lane == 0) {
      red_tail[wave] = sq;
      wcount[wave] = wbase;
    }
    __syncthreads();                                                      // [barrier 3]
    if (wave != 0) return;
    const uint32_t cw = lane < NW ? wcount[lane] : 0u;
    const double s_below = sum_partials<NW>(red_tail);
    double s_cand;
    tau = rank_candidates<NW>(cand, cw, c, rr, lane, &s_cand);
    dsum = (s_below - static_cast<double>(rank - rr) * (tau - mu_d)) + s_cand;
  } else {
    if (noisy) {
      select_exact<BLOCK, LOG_NB>(RegisterSource<Q>{d, vmask}, mu_d, rank, hist, cand, wcount,
                                  red_rng, red_tail, &tau, &dsum);
    } else {  // every sample is the nominal point: tau = its projection, no tail below it
      tau = project(h0, h1, nx, ny);
      dsum = 0.0;
    }
    if (wave != 0) return;
  }

  // ---- 5. offsets (wave 0, lane 0) -------------------------------------------------------------
  if (lane == 0) {
    const double r = prm.rc * norm_h(h0, h1);  // R_c |h| (risk_metrics.py:293, :234)
    if constexpr (METRIC)
      store_record_selected(rec, dev.selected + row * DRCVAR_SEL_WIDTH, code, mux, muy, prm.rc, h0,
                            h1, offsets_from_tail(prm, r, tau, dsum));
    else
      store_record(rec, mux, muy, prm.rc, h0, h1, offsets_from_tail(prm, r, tau, dsum));
    if (status) status[row] = failure_status(false, prm);
  }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// Launch plans: (threads, Philox pairs per thread, log2 bins); a plan holds 2 threads pairs
// samples.  Nothing has to be in flight from memory, so the blocks are wide and a thread holds few
// pairs: x, y and the generator's temporaries stay in registers.
struct Plan {
  int block, pairs, log_nb;
};
constexpr Plan kPlans[] = {
    {64, 1, 7},     // N <=   128
    {256, 1, 8},    // N <=   512
    {512, 1, 9},    // N <=  1024
    {512, 2, 10},   // N <=  2048   (two workgroups per CU: at most 128 VGPRs, see the kernel)
    {512, 4, 10},   // N <=  4096
    {512, 8, 10},   // N <=  8192
    {1024, 8, 10},  // N <= 16384
};
constexpr int kNumPlans = sizeof(kPlans) / sizeof(kPlans[0]);

int pick_plan(int64_t n) {
  for (int p = 0; p < kNumPlans; ++p)
    if (n <= int64_t{2} * kPlans[p].block * kPlans[p].pairs) return p;
  return -1;
}

struct Launch {
  const double* nominal;
  const double* ego;
  DrawArgs a;
  Params prm;
  double* out;
  int32_t* status;
  double* samples_out;
  const drcvar_step_state* state;  // non-null: the device-state form, rows clamped to path_last
  int64_t path_last;
  int64_t count;
  bool iso;
  hipStream_t stream;
  PredState pred;  // the predicted-ego form's arguments (state and path_last filled at launch)
  RiskState risk;  // the risk-table form's, likewise
  const int32_t* metric;  // the metric form's two pointers
  double* selected;
  int64_t ego_ps;  // the route form's stride
  const NoiseRow* noise;  // the noise form's table and period
  int64_t noise_period;
};

template <int BLOCK, int PP, int LOG_NB, bool ISO>
void launch_form(const Launch& L) {
  const dim3 grid(static_cast<unsigned>(L.count)), block(BLOCK);
#ifdef DRCVAR_LOOP_PRED_LIBRARY
  // this library launches the predicted-ego form alone: the only kernels it instantiates
  PredState ps = L.pred;
  ps.state = L.state;
  ps.path_last = L.path_last;
  hipLaunchKernelGGL((sampled_halfspace_kernel<BLOCK, PP, LOG_NB, ISO, true, true>), grid, block, 0,
                     L.stream, L.nominal, nullptr, L.a, L.prm, L.out, L.status, nullptr, ps);
#elif defined(DRCVAR_LOOP_RISK_LIBRARY)
  // this library launches the risk-table form alone (L.prm is not read: the rows are the table's)
  RiskState rs = L.risk;
  rs.state = L.state;
  rs.path_last = L.path_last;
  hipLaunchKernelGGL((sampled_halfspace_kernel<BLOCK, PP, LOG_NB, ISO, true, false, true>), grid,
                     block, 0, L.stream, L.nominal, L.ego, L.a, L.prm, L.out, L.status, nullptr, rs);
#elif defined(DRCVAR_LOOP_METRIC_LIBRARY)
  // this library launches the metric form alone (L.prm is not read: the rows are the table's)
  const MetricState ms{L.state, L.path_last, L.risk.table, L.risk.O, L.risk.D, L.metric, L.selected};
  hipLaunchKernelGGL((sampled_halfspace_kernel<BLOCK, PP, LOG_NB, ISO, true, false, true, true>),
                     grid, block, 0, L.stream, L.nominal, L.ego, L.a, L.prm, L.out, L.status,
                     nullptr, ms);
#elif defined(DRCVAR_LOOP_ROUTE_LIBRARY)
  // this library launches the route form alone (L.prm is not read: the rows are the table's)
  const RouteState rs{L.state, L.path_last, L.risk.table, L.risk.O, L.risk.D,
                      L.metric, L.selected, L.ego_ps};
  hipLaunchKernelGGL(
      (sampled_halfspace_kernel<BLOCK, PP, LOG_NB, ISO, true, false, true, true, true>), grid,
      block, 0, L.stream, L.nominal, L.ego, L.a, L.prm, L.out, L.status, nullptr, rs);
#elif defined(DRCVAR_LOOP_NOISE_LIBRARY)
  // this library launches the noise form alone (L.prm and L.a's factor are not read: the rows are
  // the tables')
  static_assert(!ISO, "the noise form reads the row's flag");
  const NoiseState ns{L.state, L.path_last, L.risk.table, L.risk.O, L.risk.D, L.metric,
                      L.selected, L.ego_ps, L.noise, L.noise_period};
  hipLaunchKernelGGL(
      (sampled_halfspace_kernel<BLOCK, PP, LOG_NB, false, true, false, true, true, true, true>),
      grid, block, 0, L.stream, L.nominal, L.ego, L.a, L.prm, L.out, L.status, nullptr, ns);
#else
  if (L.state)
    hipLaunchKernelGGL((sampled_halfspace_kernel<BLOCK, PP, LOG_NB, ISO, true>), grid, block, 0,
                       L.stream, L.nominal, L.ego, L.a, L.prm, L.out, L.status, nullptr,
                       DevState{L.state, L.path_last});
  else
    hipLaunchKernelGGL((sampled_halfspace_kernel<BLOCK, PP, LOG_NB, ISO, false>), grid, block, 0,
                       L.stream, L.nominal, L.ego, L.a, L.prm, L.out, L.status, L.samples_out,
                       NoState{});
#endif
}

template <int BLOCK, int PP, int LOG_NB>
void launch_plan(Launch L) {
  L.prm.hist_scale = static_cast<double>(1 << LOG_NB) / (2.0 * L.prm.window_sd);
#ifdef DRCVAR_LOOP_NOISE_LIBRARY
  launch_form<BLOCK, PP, LOG_NB, false>(L);  // one kernel per plan: the form is each row's flag
#else
  if (L.iso)
    launch_form<BLOCK, PP, LOG_NB, true>(L);
  else
    launch_form<BLOCK, PP, LOG_NB, false>(L);
#endif
}

// The sampler's test for its isotropic form (launch_samples): the draws are the same bits only if
// this kernel takes that form exactly when the sampler does.  One expression for the launch-uniform
// factor of every entry and for the rows of the noise table.
inline bool isotropic_factor(double l00, double l10, double l11) {
  const double lam = l00 * l00;
  return l10 == 0.0 && l00 == l11 && l00 > 0.0 && std::isfinite(l00) && lam >= 0x1.0p-200 &&
         lam <= 0x1.0p200;
}

// Every entry: the host checks, the launch-uniform arguments and the plan's launch.  `state`
// non-null selects the device-state form (n_steps is then the window length, path_steps the rows
// of nominal and ego; stream_offset is unused, the kernel loads it).  `pred` non-null: the
// predicted-ego form, which has no `ego`.  `risk` non-null: the risk-table form, whose five risk
// scalars here are placeholders (its Params are the table's rows).  `metric_form`: the metric form,
// a risk-table form with `metric` and `selected`; `ego_problem_stride` is read by the route
// library's build alone; `noise` and `noise_period` by the noise library's, whose l00, l10, l11 here
// are placeholders (its factors are the noise table's rows).
int sampled_halfspaces(const double* nominal, int64_t n_obstacles, int64_t n_steps, int64_t nom_so,
                       int64_t nom_st, int64_t unit_begin, int64_t unit_count, int64_t n_samples,
                       double l00, double l10, double l11, uint64_t seed, uint64_t stream_offset,
                       const drcvar_step_state* state, bool dev, int64_t path_steps,
                       int32_t zero_first_step, const double* ego, int64_t ego_stride,
                       double robot_radius, double obstacle_radius, double alpha, double delta,
                       double epsilon, double* out, int32_t* status, double* samples_out, int64_t su,
                       int64_t sn, void* stream, const PredState* pred = nullptr,
                       const RiskState* risk = nullptr, bool metric_form = false,
                       const int32_t* metric = nullptr, double* selected = nullptr,
                       int64_t ego_problem_stride = 0, const void* noise = nullptr,
                       int64_t noise_period = 1) {
  if (n_obstacles < 0 || n_steps < 0 || n_samples < 0 || unit_begin < 0 || unit_count < 0)
    return DRCVAR_ERR_INVALID_ARGUMENT;
  if (dev && path_steps < 1) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (!(l00 == l00) || !(l10 == l10) || !(l11 == l11)) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (!params_ok(robot_radius, obstacle_radius, alpha, delta, epsilon))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  // the sampler's grid limits, and the register plans' sample count
  if (n_obstacles > (int64_t{1} << 40) || n_steps > (int64_t{1} << 40) ||
      n_obstacles * n_steps > (int64_t{1} << 40) || n_samples > DRCVAR_MAX_SAMPLES)
    return DRCVAR_ERR_UNSUPPORTED;
  const int64_t units = n_obstacles * n_steps;
  if (unit_begin > units || unit_count > units - unit_begin) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (unit_count == 0 || n_samples == 0) return DRCVAR_OK;
  if (!nominal || (!ego && !pred) || !out) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (metric_form && (!metric || !selected)) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (dev && (!state || reinterpret_cast<uintptr_t>(state) % 16 != 0))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  if (unit_count > 0x7fffffffLL) return DRCVAR_ERR_UNSUPPORTED;  // one workgroup per unit: grid x
  Launch L{};
  L.nominal = nominal;
  L.ego = ego;
  L.a.T = n_steps;
  L.a.nom_so = nom_so;
  L.a.nom_st = nom_st;
  L.a.ego_st = ego_stride;
  L.a.u0 = unit_begin;
  L.a.su = su;
  L.a.sn = sn;
  L.a.n = static_cast<int>(n_samples);
  L.a.zero_first = zero_first_step != 0;
  L.a.l00 = l00;
  L.a.l10 = l10;
  L.a.l11 = l11;
  // (the device-state form replaces all but the key words in the kernel)
  L.a.pu = make_philox_uniform(static_cast<uint32_t>(stream_offset),
                               static_cast<uint32_t>(stream_offset >> 32),
                               static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
  L.iso = isotropic_factor(l00, l10, l11);
  L.a.lg = make_log_scale(L.iso ? l00 * l00 : 1.0);
  L.prm = make_params(robot_radius, obstacle_radius, alpha, delta, epsilon, n_samples);
  L.out = out;
  L.status = status;
  L.samples_out = samples_out;
  L.state = dev ? state : nullptr;
  L.path_last = path_steps - 1;
  L.count = unit_count;
  L.stream = static_cast<hipStream_t>(stream);
  if (pred) L.pred = *pred;
  if (risk) L.risk = *risk;
  L.metric = metric;
  L.selected = selected;
  L.ego_ps = ego_problem_stride;
  L.noise = static_cast<const NoiseRow*>(noise);
  L.noise_period = noise_period;
  (void)hipGetLastError();  // clear stale errors from unrelated work
  switch (pick_plan(n_samples)) {
    case 0: launch_plan<64, 1, 7>(L); break;
    case 1: launch_plan<256, 1, 8>(L); break;
    case 2: launch_plan<512, 1, 9>(L); break;
    case 3: launch_plan<512, 2, 10>(L); break;
    case 4: launch_plan<512, 4, 10>(L); break;
    case 5: launch_plan<512, 8, 10>(L); break;
    case 6: launch_plan<1024, 8, 10>(L); break;
    default: return DRCVAR_ERR_UNSUPPORTED;
  }
  return hipGetLastError() == hipSuccess ? DRCVAR_OK : DRCVAR_ERR_LAUNCH;
}

}  // namespace

#ifdef DRCVAR_LOOP_PRED_LIBRARY
extern "C" int drcvar_sampled_halfspaces_f64_pred(
    const double* nominal_path, int64_t n_obstacles, int64_t path_steps, int64_t nom_so,
    int64_t nom_st, int64_t n_steps, int64_t unit_begin, int64_t unit_count, int64_t n_samples,
    double l00, double l10, double l11, uint64_t seed, const drcvar_step_state* state,
    int32_t zero_first_step, int64_t n_obstacles_per_problem, const double* x0, const double* pred,
    int64_t pred_rows, int32_t n_states, const double* c_out, int32_t shift, double robot_radius,
    double obstacle_radius, double alpha, double delta, double epsilon, double* out,
    int32_t* status, void* stream) {
  if (n_states < 1 || n_states > kMaxStates || n_obstacles_per_problem < 1 || pred_rows < 1 ||
      (shift != 0 && shift != 1))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  // whole problems: b = (u / T) / O must stay below the rows of x0 and pred
  if (n_obstacles > 0 && n_obstacles % n_obstacles_per_problem != 0)
    return DRCVAR_ERR_INVALID_ARGUMENT;
  PredState ps{};
  const bool launches = unit_count > 0 && n_samples > 0;
  if (launches && (!x0 || !pred || !c_out)) return DRCVAR_ERR_INVALID_ARGUMENT;
  ps.x0 = x0;
  ps.pred = pred;
  ps.O = n_obstacles_per_problem;
  ps.pred_last = pred_rows - 1;
  ps.nx = n_states;
  ps.shift = shift;
  if (launches)
    for (int j = 0; j < n_states; ++j) {  // copied at call time: c_out is host memory
      ps.cx[j] = c_out[j];
      ps.cy[j] = c_out[n_states + j];
    }
  return sampled_halfspaces(nominal_path, n_obstacles, n_steps, nom_so, nom_st, unit_begin,
                            unit_count, n_samples, l00, l10, l11, seed, 0, state, true, path_steps,
                            zero_first_step, nullptr, 0, robot_radius, obstacle_radius, alpha, delta,
                            epsilon, out, status, nullptr, 0, 0, stream, &ps);
}
#elif defined(DRCVAR_LOOP_RISK_LIBRARY)
static_assert(sizeof(RiskRow) % 16 == 0, "a table row is a multiple of 16 bytes");

extern "C" int64_t drcvar_risk_table_row_bytes(void) { return static_cast<int64_t>(sizeof(RiskRow)); }

extern "C" int drcvar_risk_table_fill(const double* alpha, const double* delta,
                                      const double* epsilon, int64_t n_problems,
                                      double robot_radius, double obstacle_radius,
                                      int64_t n_samples, void* table_host, int64_t table_bytes) {
  if (n_problems < 0 || table_bytes < 0) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (n_samples < 1 || n_samples > DRCVAR_MAX_SAMPLES) return DRCVAR_ERR_UNSUPPORTED;
  if (n_problems == 0) return DRCVAR_OK;
  if (!alpha || !delta || !epsilon || !table_host) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (n_problems > table_bytes / static_cast<int64_t>(sizeof(RiskRow)))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  for (int64_t b = 0; b < n_problems; ++b)  // every row first: a rejected row writes nothing
    if (!params_ok(robot_radius, obstacle_radius, alpha[b], delta[b], epsilon[b]))
      return DRCVAR_ERR_INVALID_ARGUMENT;
  const double bins = static_cast<double>(1 << kPlans[pick_plan(n_samples)].log_nb);
  for (int64_t b = 0; b < n_problems; ++b) {
    RiskRow row;
    std::memset(&row, 0, sizeof(row));  // the padding too: equal triples give equal bytes
    row.p = make_params(robot_radius, obstacle_radius, alpha[b], delta[b], epsilon[b], n_samples);
    row.p.hist_scale = bins / (2.0 * row.p.window_sd);  // as launch_plan sets it
    std::memcpy(static_cast<char*>(table_host) + b * sizeof(RiskRow), &row, sizeof(row));
  }
  return DRCVAR_OK;
}

extern "C" int drcvar_sampled_halfspaces_f64_risk(
    const double* nominal_path, int64_t n_obstacles, int64_t path_steps, int64_t nom_so,
    int64_t nom_st, int64_t n_steps, int64_t unit_begin, int64_t unit_count, int64_t n_samples,
    double l00, double l10, double l11, uint64_t seed, const drcvar_step_state* state,
    int32_t zero_first_step, const double* ego_path, int64_t ego_stride,
    int64_t n_obstacles_per_problem, const void* table, int64_t draw_period, double* out,
    int32_t* status, void* stream) {
  if (n_obstacles_per_problem < 1 || draw_period < 1) return DRCVAR_ERR_INVALID_ARGUMENT;
  // whole problems: b = (u / T) / O must stay below the rows of the table
  if (n_obstacles > 0 && n_obstacles % n_obstacles_per_problem != 0)
    return DRCVAR_ERR_INVALID_ARGUMENT;
  const bool launches = unit_count > 0 && n_samples > 0;
  if (launches && (!table || reinterpret_cast<uintptr_t>(table) % 16 != 0))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  RiskState rs{};
  rs.table = static_cast<const RiskRow*>(table);
  rs.O = n_obstacles_per_problem;
  rs.D = draw_period;
  // (placeholder risk scalars that params_ok accepts: the kernel reads the table's rows)
  return sampled_halfspaces(nominal_path, n_obstacles, n_steps, nom_so, nom_st, unit_begin,
                            unit_count, n_samples, l00, l10, l11, seed, 0, state, true, path_steps,
                            zero_first_step, ego_path, ego_stride, 0.0, 0.0, 1.0, 0.0, 0.0, out,
                            status, nullptr, 0, 0, stream, nullptr, &rs);
}
#elif defined(DRCVAR_LOOP_METRIC_LIBRARY)
// (the rows are drcvar_risk_table_fill's, made from this source: include/drcvar_loop_risk.h)
extern "C" int64_t drcvar_metric_table_row_bytes(void) { return static_cast<int64_t>(sizeof(RiskRow)); }

extern "C" int drcvar_sampled_halfspaces_f64_metric(
    const double* nominal_path, int64_t n_obstacles, int64_t path_steps, int64_t nom_so,
    int64_t nom_st, int64_t n_steps, int64_t unit_begin, int64_t unit_count, int64_t n_samples,
    double l00, double l10, double l11, uint64_t seed, const drcvar_step_state* state,
    int32_t zero_first_step, const double* ego_path, int64_t ego_stride,
    int64_t n_obstacles_per_problem, const void* table, int64_t draw_period, const int32_t* metric,
    double* out, int32_t* status, double* selected, void* stream) {
  // the risk-table entry's checks, in its order; metric and selected beside nominal_path's
  if (n_obstacles_per_problem < 1 || draw_period < 1) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (n_obstacles > 0 && n_obstacles % n_obstacles_per_problem != 0)
    return DRCVAR_ERR_INVALID_ARGUMENT;
  const bool launches = unit_count > 0 && n_samples > 0;
  if (launches && (!table || reinterpret_cast<uintptr_t>(table) % 16 != 0))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  RiskState rs{};
  rs.table = static_cast<const RiskRow*>(table);
  rs.O = n_obstacles_per_problem;
  rs.D = draw_period;
  return sampled_halfspaces(nominal_path, n_obstacles, n_steps, nom_so, nom_st, unit_begin,
                            unit_count, n_samples, l00, l10, l11, seed, 0, state, true, path_steps,
                            zero_first_step, ego_path, ego_stride, 0.0, 0.0, 1.0, 0.0, 0.0, out,
                            status, nullptr, 0, 0, stream, nullptr, &rs, true, metric, selected);
}
#elif defined(DRCVAR_LOOP_ROUTE_LIBRARY)
extern "C" int drcvar_sampled_halfspaces_f64_route(
    const double* nominal_path, int64_t n_obstacles, int64_t path_steps, int64_t nom_so,
    int64_t nom_st, int64_t n_steps, int64_t unit_begin, int64_t unit_count, int64_t n_samples,
    double l00, double l10, double l11, uint64_t seed, const drcvar_step_state* state,
    int32_t zero_first_step, const double* ego_path, int64_t ego_stride,
    int64_t ego_problem_stride, int64_t n_obstacles_per_problem, const void* table,
    int64_t draw_period, const int32_t* metric, double* out, int32_t* status, double* selected,
    void* stream) {
  // the stride first, then the metric entry's checks in its order
  if (ego_problem_stride < 0) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (ego_problem_stride > (int64_t{1} << 40)) return DRCVAR_ERR_UNSUPPORTED;
  if (n_obstacles_per_problem < 1 || draw_period < 1) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (n_obstacles > 0 && n_obstacles % n_obstacles_per_problem != 0)
    return DRCVAR_ERR_INVALID_ARGUMENT;
  const bool launches = unit_count > 0 && n_samples > 0;
  if (launches && (!table || reinterpret_cast<uintptr_t>(table) % 16 != 0))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  RiskState rs{};
  rs.table = static_cast<const RiskRow*>(table);
  rs.O = n_obstacles_per_problem;
  rs.D = draw_period;
  return sampled_halfspaces(nominal_path, n_obstacles, n_steps, nom_so, nom_st, unit_begin,
                            unit_count, n_samples, l00, l10, l11, seed, 0, state, true, path_steps,
                            zero_first_step, ego_path, ego_stride, 0.0, 0.0, 1.0, 0.0, 0.0, out,
                            status, nullptr, 0, 0, stream, nullptr, &rs, true, metric, selected,
                            ego_problem_stride);
}
#elif defined(DRCVAR_LOOP_NOISE_LIBRARY)
static_assert(sizeof(NoiseRow) % 16 == 0, "a noise row is a multiple of 16 bytes");

extern "C" int64_t drcvar_noise_table_row_bytes(void) { return static_cast<int64_t>(sizeof(NoiseRow)); }

extern "C" int drcvar_noise_table_fill(const double* chol, int64_t rows, void* out,
                                       int64_t out_bytes) {
  if (rows < 0 || out_bytes < 0) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (rows == 0) return DRCVAR_OK;
  if (!chol || !out) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (rows > out_bytes / static_cast<int64_t>(sizeof(NoiseRow))) return DRCVAR_ERR_INVALID_ARGUMENT;
  for (int64_t r = 0; r < 3 * rows; ++r)  // every row first: a rejected row writes nothing
    if (!(chol[r] == chol[r])) return DRCVAR_ERR_INVALID_ARGUMENT;
  for (int64_t r = 0; r < rows; ++r) {
    NoiseRow row;
    std::memset(&row, 0, sizeof(row));  // equal factors give equal bytes
    row.l00 = chol[3 * r];
    row.l10 = chol[3 * r + 1];
    row.l11 = chol[3 * r + 2];
    const bool iso = isotropic_factor(row.l00, row.l10, row.l11);
    row.iso = iso ? 1 : 0;
    row.lg = make_log_scale(iso ? row.l00 * row.l00 : 1.0);  // as sampled_halfspaces sets a.lg
    std::memcpy(static_cast<char*>(out) + r * sizeof(NoiseRow), &row, sizeof(row));
  }
  return DRCVAR_OK;
}

extern "C" int drcvar_sampled_halfspaces_f64_noise(
    const double* nominal_path, int64_t n_obstacles, int64_t path_steps, int64_t nom_so,
    int64_t nom_st, int64_t n_steps, int64_t unit_begin, int64_t unit_count, int64_t n_samples,
    const void* noise, int64_t noise_period, uint64_t seed, const drcvar_step_state* state,
    int32_t zero_first_step, const double* ego_path, int64_t ego_stride,
    int64_t ego_problem_stride, int64_t n_obstacles_per_problem, const void* table,
    int64_t draw_period, const int32_t* metric, double* out, int32_t* status, double* selected,
    void* stream) {
  // the noise table first (row (o mod noise_period) T + t stays inside noise_period T rows for
  // every o), then the route entry's checks in its order
  if (noise_period < 1 || noise_period > n_obstacles) return DRCVAR_ERR_INVALID_ARGUMENT;
  const bool launches = unit_count > 0 && n_samples > 0;
  if (launches && (!noise || reinterpret_cast<uintptr_t>(noise) % 16 != 0))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  if (ego_problem_stride < 0) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (ego_problem_stride > (int64_t{1} << 40)) return DRCVAR_ERR_UNSUPPORTED;
  if (n_obstacles_per_problem < 1 || draw_period < 1) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (n_obstacles > 0 && n_obstacles % n_obstacles_per_problem != 0)
    return DRCVAR_ERR_INVALID_ARGUMENT;
  if (launches && (!table || reinterpret_cast<uintptr_t>(table) % 16 != 0))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  RiskState rs{};
  rs.table = static_cast<const RiskRow*>(table);
  rs.O = n_obstacles_per_problem;
  rs.D = draw_period;
  // (a placeholder factor that the NaN check accepts: the kernel reads the noise table's rows)
  return sampled_halfspaces(nominal_path, n_obstacles, n_steps, nom_so, nom_st, unit_begin,
                            unit_count, n_samples, 0.0, 0.0, 0.0, seed, 0, state, true, path_steps,
                            zero_first_step, ego_path, ego_stride, 0.0, 0.0, 1.0, 0.0, 0.0, out,
                            status, nullptr, 0, 0, stream, nullptr, &rs, true, metric, selected,
                            ego_problem_stride, noise, noise_period);
}
#else
extern "C" int drcvar_sampled_launch_plan(int64_t n_samples, int32_t* threads,
                                          int32_t* pairs_per_thread) {
  if (n_samples < 1) return DRCVAR_ERR_INVALID_ARGUMENT;
  const int p = pick_plan(n_samples);
  if (p < 0) return DRCVAR_ERR_UNSUPPORTED;
  if (threads) *threads = kPlans[p].block;
  if (pairs_per_thread) *pairs_per_thread = kPlans[p].pairs;
  return DRCVAR_OK;
}

extern "C" int drcvar_sampled_halfspaces_f64(
    const double* nominal, int64_t n_obstacles, int64_t n_steps, int64_t nom_so, int64_t nom_st,
    int64_t unit_begin, int64_t unit_count, int64_t n_samples, double l00, double l10, double l11,
    uint64_t seed, uint64_t stream_offset, int32_t zero_first_step, const double* ego,
    int64_t ego_stride, double robot_radius, double obstacle_radius, double alpha, double delta,
    double epsilon, double* out, int32_t* status, double* samples_out, int64_t su, int64_t sn,
    void* stream) {
  return sampled_halfspaces(nominal, n_obstacles, n_steps, nom_so, nom_st, unit_begin, unit_count,
                            n_samples, l00, l10, l11, seed, stream_offset, nullptr, false, 0,
                            zero_first_step, ego, ego_stride, robot_radius, obstacle_radius, alpha,
                            delta, epsilon, out, status, samples_out, su, sn, stream);
}

extern "C" int drcvar_sampled_halfspaces_f64_dev(
    const double* nominal_path, int64_t n_obstacles, int64_t path_steps, int64_t nom_so,
    int64_t nom_st, int64_t n_steps, int64_t unit_begin, int64_t unit_count, int64_t n_samples,
    double l00, double l10, double l11, uint64_t seed, const drcvar_step_state* state,
    int32_t zero_first_step, const double* ego_path, int64_t ego_stride, double robot_radius,
    double obstacle_radius, double alpha, double delta, double epsilon, double* out,
    int32_t* status, void* stream) {
  return sampled_halfspaces(nominal_path, n_obstacles, n_steps, nom_so, nom_st, unit_begin,
                            unit_count, n_samples, l00, l10, l11, seed, 0, state, true, path_steps,
                            zero_first_step, ego_path, ego_stride, robot_radius, obstacle_radius,
                            alpha, delta, epsilon, out, status, nullptr, 0, 0, stream);
}
#endif
