// drcvar_clearance.hip — Monte Carlo out-of-sample collision evaluation, for gfx950.
//
// Reference: main.py:128-138 draws ONE Laplace realisation per obstacle
// (simulation/obstacles.py:79-113) and takes each filtered trajectory's per-step clearance from it
// (simulation/environment.py:108-140).  A collision rate of 1e-3 needs 1e5-1e7 realisations; this
// kernel draws M of them and reduces each to a clearance without writing a realisation to memory:
//
//   thread = realisation m; loop t outer, o inner: one Philox4x32-10 call per (m, o, t), counter
//   g = m (O T) + o T + t -> noise (Laplace: bx (E(x0) - E(x1)), by (E(x2) - E(x3)), E = -log u32;
//   Gaussian: Box-Muller of (x0, x1), L z) -> obstacle position -> d^2 to each of the K ego
//   trajectories (all K see the same draw: common random numbers, and the generator's cost is
//   divided by K) -> K running minima of d^2 in registers.
//
// ego[k, t] and nominal[o, t] are wave-uniform (restrict-qualified kernel arguments: scalar loads),
// the generator's tables are in LDS as in the sampler (drcvar_generator.inc, included unedited).
// Outputs: min_clearance[k, m] = sqrt(min d^2) - R, one sqrt at the end, and optionally
// step_hits[k, t] = #{m : min_o d^2 < R^2} (one ballot + popcount per wave and (k, t), one integer
// atomic add by one lane when the count is not zero).
//
// Small M with a large O T grid leaves the device empty, so grid.y splits the step range.  With
// more than one split the output is first filled with all-ones bytes, every split combines its
// partial minimum by an unsigned 64-bit atomic min on a key, the bit pattern of the non-negative
// d^2 plus one (the order of non-negative doubles is the order of their bit patterns: exact,
// independent of arrival order) or 0 for NaN, which so wins, and a finishing launch decodes the key
// and applies sqrt - R in place.  One split stores directly.  Both paths take the minimum of the
// same d^2 values and apply the same sqrt: the same bits.
//
// Non-finite positions follow IEEE 754 as the NumPy mirror of these formulas does (the contract is
// in drcvar_sampling.h): a NaN d^2 makes its clearance NaN and its step count nothing.  v_min_f64
// alone would drop it; max_high below carries it.
//
// The source is compiled twice.  Into the engine library: the kernel above behind
// drcvar_min_clearance_f64[_ex].  With DRCVAR_LOOP_EVAL_LIBRARY into a library of its own
// (include/drcvar_loop_eval.h): the device-state, batched, one-row form for receding-horizon
// loops replayed from a graph (loop_clearance_kernel below).  Both draw with draw_noise and form
// the obstacle point and d^2 by the same expressions.  (A shared inline helper for those four lines
// changed the first kernel's instruction schedule, so they are written out in both.)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "drcvar_sampling.h"
#ifdef DRCVAR_LOOP_EVAL_LIBRARY
#include "drcvar_loop_eval.h"
#endif

namespace {

constexpr int kBlock = 256;
constexpr int kMaxTraj = 8;
// Workgroups wanted before the step range stops being split further: four per CU of the 256.
constexpr int64_t kWantedGroups = 1024;

#include "drcvar_generator.inc"

struct ClearArgs {
  int64_t ego_sk, ego_st, nom_so, nom_st;
  int64_t O, T, OT;
  int64_t m_begin, M;
  double p0, p1, p2;  // Gaussian: l00, l10, l11; Laplace: bx, by
  double R, RR;
  PhiloxUniform pu;
  LogScale lg;
  int zero_first;
  int64_t out_sk;
  int64_t steps_per_split;
};

// The noise of one (m, o, t) from its Philox call.  kLaplace: the log carries lam = 1/2, so
// scaled_neg2_log_u32 is E = -log u; otherwise lam = 1 and (x0, x1) are Box-Muller's radius and
// angle words (x2, x3 unused).
// Args: a kernel's argument struct with p0, p1, p2, pu and lg.
template <bool kLaplace, class Args>
__device__ __forceinline__ void draw_noise(uint64_t g, const Args& a, const double* s_turn,
                                           const double* s_log, double* nx, double* ny) {
  const Philox r = philox4x32_10(static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32), a.pu);
  if constexpr (kLaplace) {
    const double e0 = scaled_neg2_log_u32(r.x[0], s_log, a.lg);
    const double e1 = scaled_neg2_log_u32(r.x[1], s_log, a.lg);
    const double e2 = scaled_neg2_log_u32(r.x[2], s_log, a.lg);
    const double e3 = scaled_neg2_log_u32(r.x[3], s_log, a.lg);
    *nx = a.p0 * (e0 - e1);
    *ny = a.p1 * (e2 - e3);
  } else {
    double cs, sn;
    const double rad = sqrt_normal(scaled_neg2_log_u32(r.x[0], s_log, a.lg));
    cos_sin_u32(r.x[1], s_turn, &cs, &sn);
    const double z0 = rad * cs, z1 = rad * sn;
    *nx = a.p0 * z0;
    *ny = fma(a.p1, z0, a.p2 * z1);
  }
}

// min(a, b) as one v_min_f64: the builtin's lowering first canonicalises each loop-carried operand
// (a v_max_f64 x, x apiece), two more VALU instructions per trajectory and point.
__device__ __forceinline__ double min_f64(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// v_min_f64 returns the other operand when one is a quiet NaN, so a NaN d^2 would drop out of
// every minimum.  It is carried beside the minimum instead: an unsigned maximum of the high words
// of the d^2 values (one v_max_u32 per trajectory and point).  A d^2 = fma(dx, dx, dy * dy) is
// either >= +0 (high word at most that of +inf) or a NaN that the fma has quieted (high word, with
// or without the sign, above kInfHigh): the maximum is above kInfHigh exactly when a member is NaN.
constexpr uint32_t kInfHigh = 0x7ff00000u;
__device__ __forceinline__ uint32_t max_high(uint32_t h, double d2) {
  const uint32_t w = static_cast<uint32_t>(__double2hiint(d2));
  return h > w ? h : w;
}

#ifndef DRCVAR_LOOP_EVAL_LIBRARY
template <int K, bool kLaplace>
__global__ __launch_bounds__(kBlock) void clearance_kernel(const double* __restrict__ ego,
                                                           const double* __restrict__ nominal,
                                                           double* __restrict__ out,
                                                           unsigned long long* __restrict__ hits,
                                                           ClearArgs a) {
  __shared__ double s_turn[kTurnLen], s_log[2 * kLogIdx];
  load_generator_tables(s_turn, s_log, kBlock, a.lg.lam);
  __syncthreads();
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const bool valid = i < a.M;
  // a lane past M draws realisation m_begin (no index depends on it) and neither stores nor counts
  const uint64_t gm = static_cast<uint64_t>(a.m_begin + (valid ? i : 0)) * static_cast<uint64_t>(a.OT);
  const int64_t t0 = static_cast<int64_t>(blockIdx.y) * a.steps_per_split;
  const int64_t t1 = t0 + a.steps_per_split < a.T ? t0 + a.steps_per_split : a.T;
  const double inf = std::numeric_limits<double>::infinity();
  double mn[K];
  uint32_t nan_met = 0;  // bit k: some d^2 of trajectory k was NaN
#pragma unroll
  for (int k = 0; k < K; ++k) mn[k] = inf;
  for (int64_t t = t0; t < t1; ++t) {
    double ex[K], ey[K], mo[K];
    uint32_t ho[K];  // max_high over this step's d^2 of trajectory k
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double* e = ego + k * a.ego_sk + t * a.ego_st;
      ex[k] = e[0];
      ey[k] = e[1];
      mo[k] = inf;
      ho[k] = 0;
    }
    const bool noisy = !(a.zero_first && t == 0);  // the noise-free first step: no Philox call
    const double* nom = nominal + t * a.nom_st;
    uint64_t ot = static_cast<uint64_t>(t);         // o T + t
    for (int64_t o = 0; o < a.O; ++o, nom += a.nom_so, ot += static_cast<uint64_t>(a.T)) {
      double nx = 0.0, ny = 0.0;
      if (noisy) draw_noise<kLaplace>(gm + ot, a, s_turn, s_log, &nx, &ny);
      const double px = nom[0] + nx, py = nom[1] + ny;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double dx = ex[k] - px, dy = ey[k] - py;
        const double d2 = fma(dx, dx, dy * dy);
        mo[k] = min_f64(mo[k], d2);
        ho[k] = max_high(ho[k], d2);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      mn[k] = min_f64(mn[k], mo[k]);
      nan_met |= static_cast<uint32_t>(ho[k] > kInfHigh) << k;
      if (hits) {
        // a minimum with a NaN member is NaN and counts nothing
        const unsigned long long hit =
            __builtin_amdgcn_ballot_w64(valid && mo[k] < a.RR && ho[k] <= kInfHigh);
        if (hit != 0 && (threadIdx.x & 63) == 0)
          atomicAdd(hits + k * a.T + t, static_cast<unsigned long long>(__builtin_popcountll(hit)));
      }
    }
  }
  if (!valid) return;
  if (gridDim.y == 1) {
#pragma unroll
    for (int k = 0; k < K; ++k)
      out[k * a.out_sk + i] = (nan_met >> k & 1u) ? std::numeric_limits<double>::quiet_NaN()
                                                  : __builtin_sqrt(mn[k]) - a.R;
  } else {
    // key: 0 for NaN (it wins every atomic min), else the bit pattern of min d^2 >= +0 plus one
    // (at most that of +inf plus one: below the all-ones fill)
#pragma unroll
    for (int k = 0; k < K; ++k)
      atomicMin(reinterpret_cast<unsigned long long*>(out + k * a.out_sk + i),
                (nan_met >> k & 1u) ? 0ull
                                    : static_cast<unsigned long long>(__double_as_longlong(mn[k])) + 1ull);
  }
}

// The split form's last pass: out[k, i] holds the key of min d^2 (its bit pattern plus one; 0 where
// a split met a NaN; all-ones where no split wrote: the empty O T grid), replaced in place by
// sqrt - R, or by NaN.
__global__ __launch_bounds__(kBlock) void clearance_finish_kernel(double* out, int64_t out_sk,
                                                                  int64_t M, double R) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= M) return;
  double* p = out + blockIdx.y * out_sk + i;
  const long long key = __double_as_longlong(*p);
  const double d2 = key == -1LL ? std::numeric_limits<double>::infinity() : __longlong_as_double(key - 1);
  *p = key == 0 ? std::numeric_limits<double>::quiet_NaN() : __builtin_sqrt(d2) - R;
}

template <bool kLaplace>
void launch_for_k(int K, dim3 grid, hipStream_t s, const double* ego, const double* nominal,
                  double* out, unsigned long long* hits, const ClearArgs& a) {
  switch (K) {
#define DRCVAR_CLEARANCE_CASE(k)                                                                    \
  case k:                                                                                           \
    hipLaunchKernelGGL((clearance_kernel<k, kLaplace>), grid, dim3(kBlock), 0, s, ego, nominal, out, \
                       hits, a);                                                                    \
    break;
    DRCVAR_CLEARANCE_CASE(1)
    DRCVAR_CLEARANCE_CASE(2)
    DRCVAR_CLEARANCE_CASE(3)
    DRCVAR_CLEARANCE_CASE(4)
    DRCVAR_CLEARANCE_CASE(5)
    DRCVAR_CLEARANCE_CASE(6)
    DRCVAR_CLEARANCE_CASE(7)
    DRCVAR_CLEARANCE_CASE(8)
#undef DRCVAR_CLEARANCE_CASE
  }
}

#else  // DRCVAR_LOOP_EVAL_LIBRARY: the device-state, batched, one-row form

// One launch evaluates the CURRENT state of each of B loops: O points per (problem, realisation)
// where the kernel above has O T.  blockIdx.y = problem b, so state[b], x0[b] and the obstacles'
// nominal row are uniform over the workgroup (scalar loads), and the table load is paid once per
// workgroup: a thread takes per_thread realisations, kBlock apart (coalesced min_d2 rows), and
// blockIdx.x picks the chunk of per_thread kBlock realisations.  Exactly one thread owns (b, m) in
// a launch: the running minimum is a load, a v_min_f64 and a store (NaN kept: max_high above),
// ordered against the previous control step's launch by the stream alone.  The hit count of a wave is summed over its
// realisations in a scalar register (one ballot and popcount each) and leaves as at most one
// integer atomic add.  Nothing depends on per_thread or the grid but which thread owns (b, m).
constexpr int kMaxStates = 8;           // DRCVAR_MPC_MAX_STATES
constexpr int kRulePerThread = 8;       // the most realisations per thread the rule below chooses
constexpr int kMaxPerThread = 64;       // ... and the most a caller may ask for
constexpr int64_t kWantedLoopGroups = 2048;  // workgroups before a thread takes more realisations

struct LoopEvalArgs {
  int64_t nom_so, nom_st, O, Tn, OT, path_last, step_begin, log_rows, M, out_sb;
  uint64_t eval_offset, offset_stride;
  uint32_t k0, k1;  // the seed's words
  int nx, zero_first, per_thread;
  double cx[kMaxStates], cy[kMaxStates];  // c_out's two rows, zero past nx
  double p0, p1, p2, RR;
  LogScale lg;
};

// what draw_noise takes (ClearArgs' noise members)
struct NoiseArgs {
  double p0, p1, p2;
  PhiloxUniform pu;
  LogScale lg;
};

template <bool kLaplace>
__global__ __launch_bounds__(kBlock) void loop_clearance_kernel(
    const double* __restrict__ x0, const double* __restrict__ nominal,
    const drcvar_step_state* __restrict__ state, double* __restrict__ min_d2,
    unsigned long long* __restrict__ hits, LoopEvalArgs a) {
  __shared__ double s_turn[kTurnLen], s_log[2 * kLogIdx];
  const int64_t b = blockIdx.y;
  const int64_t s = state[b].step;
  // i = s - step_begin in wrapping arithmetic, as the advance kernel forms it; the state just
  // reached is log row i, so i = log_rows is still a row
  const uint64_t i = static_cast<uint64_t>(s) - static_cast<uint64_t>(a.step_begin);
  if (i > static_cast<uint64_t>(a.log_rows) || s < 0 || s >= a.Tn) return;  // (the whole workgroup)
  load_generator_tables(s_turn, s_log, kBlock, a.lg.lam);
  __syncthreads();
  // ego = c_out x0[b]: an fma chain from +0.0 over the states
  double ex = 0.0, ey = 0.0;
  const double* xb = x0 + b * a.nx;
#pragma unroll
  for (int j = 0; j < kMaxStates; ++j) {
    if (j < a.nx) {
      const double xj = xb[j];
      ex = fma(a.cx[j], xj, ex);
      ey = fma(a.cy[j], xj, ey);
    }
  }
  const uint64_t words = a.eval_offset + static_cast<uint64_t>(b) * a.offset_stride;  // mod 2^64
  NoiseArgs n;
  n.p0 = a.p0;
  n.p1 = a.p1;
  n.p2 = a.p2;
  n.pu = make_philox_uniform(static_cast<uint32_t>(words), static_cast<uint32_t>(words >> 32), a.k0, a.k1);
  n.lg = a.lg;
  const bool noisy = !(a.zero_first && s == 0);  // the noise-free first step: no Philox call
  const int64_t row = s < a.path_last ? s : a.path_last;
  const double* nom_b = nominal + b * a.O * a.nom_so + row * a.nom_st;
  double* out = min_d2 + b * a.out_sb;
  const int wave_first = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) & ~63);
  const int64_t chunk = static_cast<int64_t>(blockIdx.x) * a.per_thread * kBlock;
  const double inf = std::numeric_limits<double>::infinity();
  unsigned int count = 0;  // this wave's realisations in collision (uniform over the wave)
  for (int r = 0; r < a.per_thread; ++r) {
    const int64_t first = chunk + static_cast<int64_t>(r) * kBlock;
    if (first + wave_first >= a.M) break;  // nothing left for this wave
    const int64_t m = first + threadIdx.x;
    const bool valid = m < a.M;
    // a lane past M draws realisation 0 (no index depends on it) and neither stores nor counts
    const uint64_t gm = static_cast<uint64_t>(valid ? m : 0) * static_cast<uint64_t>(a.OT);
    double mo = inf;
    uint32_t ho = 0;  // max_high over this launch's d^2(m, o)
    const double* nom = nom_b;
    uint64_t ot = static_cast<uint64_t>(s);  // o T_n + s
    for (int64_t o = 0; o < a.O; ++o, nom += a.nom_so, ot += static_cast<uint64_t>(a.Tn)) {
      double nx = 0.0, ny = 0.0;
      if (noisy) draw_noise<kLaplace>(gm + ot, n, s_turn, s_log, &nx, &ny);
      const double px = nom[0] + nx, py = nom[1] + ny;
      const double dx = ex - px, dy = ey - py;
      const double d2 = fma(dx, dx, dy * dy);
      mo = min_f64(mo, d2);
      ho = max_high(ho, d2);
    }
    // a NaN met now is stored, a NaN stored by an earlier launch stays; this launch's count
    // depends on this launch's d^2 alone
    if (valid) {
      const double prev = out[m];
      out[m] = (ho > kInfHigh || prev != prev) ? std::numeric_limits<double>::quiet_NaN()
                                               : min_f64(prev, mo);
    }
    if (hits)
      count += __builtin_popcountll(__builtin_amdgcn_ballot_w64(valid && mo < a.RR && ho <= kInfHigh));
  }
  if (hits && count != 0 && (threadIdx.x & 63) == 0)
    __hip_atomic_fetch_add(hits + b * (a.log_rows + 1) + static_cast<int64_t>(i),
                           static_cast<unsigned long long>(count), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}
#endif

}  // namespace

#ifdef DRCVAR_LOOP_EVAL_LIBRARY
extern "C" int drcvar_loop_clearance_f64_ex(
    int64_t n_problems, const double* x0, int32_t n_states, const double* c_out,
    const double* nominal_path, int64_t n_obstacles, int64_t path_steps, int64_t nom_so,
    int64_t nom_st, const drcvar_step_state* state, int64_t step_begin, int64_t log_rows,
    int64_t noise_steps, int32_t noise_kind, double p0, double p1, double p2, double combined_radius,
    int64_t n_realizations, uint64_t seed, uint64_t eval_offset, uint64_t problem_offset_stride,
    int32_t zero_first_step, double* min_d2, int64_t out_sb, int64_t* step_hits,
    int32_t realizations_per_thread, void* stream) {
  if (n_problems < 0 || n_obstacles < 0 || n_realizations < 0 || noise_steps < 0 ||
      realizations_per_thread < 0 || (noise_kind != 0 && noise_kind != 1))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  if (!std::isfinite(p0) || !std::isfinite(p1) || !std::isfinite(p2) || !(combined_radius >= 0.0))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  if (noise_kind == 1 && (p0 < 0.0 || p1 < 0.0)) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (n_states < 1 || n_states > kMaxStates || path_steps < 1 || log_rows < 0)
    return DRCVAR_ERR_INVALID_ARGUMENT;
  if (n_problems == 0 || n_realizations == 0 || n_obstacles == 0) return DRCVAR_OK;  // no launch
  if (!x0 || !c_out || !nominal_path || !state || !min_d2 ||
      reinterpret_cast<uintptr_t>(state) % 16 != 0)
    return DRCVAR_ERR_INVALID_ARGUMENT;
  constexpr int64_t kMaxUnits = int64_t{1} << 20, kMaxReal = int64_t{1} << 40;
  if (n_obstacles > kMaxUnits || noise_steps > kMaxUnits || n_obstacles * noise_steps > kMaxUnits ||
      n_realizations > kMaxReal || realizations_per_thread > kMaxPerThread || n_problems > 65535)
    return DRCVAR_ERR_UNSUPPORTED;
  if (noise_steps == 0) return DRCVAR_OK;  // no step lies in [0, noise_steps): nothing is evaluated
  const int64_t M = n_realizations, blocks = (M + kBlock - 1) / kBlock;
  // Realisations per thread: one while the launch has fewer than kWantedLoopGroups workgroups
  // (eight per CU: what is resident at once), then as many as keep that number, at most
  // kRulePerThread; spread evenly over the chunks, so that the last one is not mostly empty.
  // Measured: at B = 1024, M = 10000 the launch takes 149 us at 1 per thread,
  // 128-129 us at 4 and 8, 142 us at 16 and 209 us at 32; at B <= 64 more than 2 only costs.
  int64_t per = realizations_per_thread;
  if (per == 0) {
    per = std::min<int64_t>(std::max<int64_t>(n_problems * blocks / kWantedLoopGroups, 1), kRulePerThread);
    const int64_t chunks = (blocks + per - 1) / per;
    per = (blocks + chunks - 1) / chunks;
  }
  const int64_t gx = (blocks + per - 1) / per;
  if (gx > 0x7fffffffLL) return DRCVAR_ERR_UNSUPPORTED;
  LoopEvalArgs a{};
  a.nom_so = nom_so;
  a.nom_st = nom_st;
  a.O = n_obstacles;
  a.Tn = noise_steps;
  a.OT = n_obstacles * noise_steps;
  a.path_last = path_steps - 1;
  a.step_begin = step_begin;
  a.log_rows = log_rows;
  a.M = M;
  a.out_sb = out_sb;
  a.eval_offset = eval_offset;
  a.offset_stride = problem_offset_stride;
  a.k0 = static_cast<uint32_t>(seed);
  a.k1 = static_cast<uint32_t>(seed >> 32);
  a.nx = n_states;
  a.zero_first = zero_first_step != 0;
  a.per_thread = static_cast<int>(per);
  for (int j = 0; j < n_states; ++j) {  // copied at call time: c_out is host memory
    a.cx[j] = c_out[j];
    a.cy[j] = c_out[n_states + j];
  }
  a.p0 = p0;
  a.p1 = p1;
  a.p2 = p2;
  a.RR = combined_radius * combined_radius;
  a.lg = make_log_scale(noise_kind == 1 ? 0.5 : 1.0);
  const dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(n_problems));
  const hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long* hits = reinterpret_cast<unsigned long long*>(step_hits);
  (void)hipGetLastError();  // clear stale errors from unrelated work
  if (noise_kind == 1)
    hipLaunchKernelGGL(loop_clearance_kernel<true>, grid, dim3(kBlock), 0, s, x0, nominal_path, state,
                       min_d2, hits, a);
  else
    hipLaunchKernelGGL(loop_clearance_kernel<false>, grid, dim3(kBlock), 0, s, x0, nominal_path, state,
                       min_d2, hits, a);
  return hipGetLastError() == hipSuccess ? DRCVAR_OK : DRCVAR_ERR_LAUNCH;
}

extern "C" int drcvar_loop_clearance_f64(
    int64_t n_problems, const double* x0, int32_t n_states, const double* c_out,
    const double* nominal_path, int64_t n_obstacles, int64_t path_steps, int64_t nom_so,
    int64_t nom_st, const drcvar_step_state* state, int64_t step_begin, int64_t log_rows,
    int64_t noise_steps, int32_t noise_kind, double p0, double p1, double p2, double combined_radius,
    int64_t n_realizations, uint64_t seed, uint64_t eval_offset, uint64_t problem_offset_stride,
    int32_t zero_first_step, double* min_d2, int64_t out_sb, int64_t* step_hits, void* stream) {
  return drcvar_loop_clearance_f64_ex(n_problems, x0, n_states, c_out, nominal_path, n_obstacles,
                                      path_steps, nom_so, nom_st, state, step_begin, log_rows,
                                      noise_steps, noise_kind, p0, p1, p2, combined_radius,
                                      n_realizations, seed, eval_offset, problem_offset_stride,
                                      zero_first_step, min_d2, out_sb, step_hits, 0, stream);
}
#else
extern "C" int drcvar_min_clearance_f64_ex(const double* ego, int64_t n_traj, int64_t ego_sk,
                                           int64_t ego_st, const double* nominal,
                                           int64_t n_obstacles, int64_t n_steps, int64_t nom_so,
                                           int64_t nom_st, int32_t noise_kind, double p0, double p1,
                                           double p2, double combined_radius, int64_t m_begin,
                                           int64_t n_realizations, uint64_t seed,
                                           uint64_t stream_offset, int32_t zero_first_step,
                                           double* min_clearance_out, int64_t out_sk,
                                           int64_t* step_hits, int32_t step_splits, void* stream) {
  if (n_traj < 0 || n_obstacles < 0 || n_steps < 0 || m_begin < 0 || n_realizations < 0 ||
      step_splits < 0 || (noise_kind != 0 && noise_kind != 1))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  if (!std::isfinite(p0) || !std::isfinite(p1) || !std::isfinite(p2) || !(combined_radius >= 0.0))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  if (noise_kind == 1 && (p0 < 0.0 || p1 < 0.0)) return DRCVAR_ERR_INVALID_ARGUMENT;
  constexpr int64_t kMaxUnits = int64_t{1} << 20, kMaxReal = int64_t{1} << 40;
  if (n_traj < 1 || n_traj > kMaxTraj || n_obstacles > kMaxUnits || n_steps > kMaxUnits ||
      n_obstacles * n_steps > kMaxUnits || m_begin > kMaxReal || n_realizations > kMaxReal - m_begin)
    return DRCVAR_ERR_UNSUPPORTED;
  const int64_t M = n_realizations, OT = n_obstacles * n_steps;
  if (M == 0 && !step_hits) return DRCVAR_OK;
  if (M > 0 && !min_clearance_out) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (OT > 0 && M > 0 && (!ego || !nominal)) return DRCVAR_ERR_INVALID_ARGUMENT;
  const int64_t gx = (M + kBlock - 1) / kBlock;
  if (gx > 0x7fffffffLL) return DRCVAR_ERR_UNSUPPORTED;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  (void)hipGetLastError();
  // the call sets step_hits (it does not accumulate into it)
  if (step_hits && n_steps > 0 &&
      hipMemsetAsync(step_hits, 0, static_cast<size_t>(n_traj * n_steps) * sizeof(int64_t), s) != hipSuccess)
    return DRCVAR_ERR_LAUNCH;
  if (M == 0) return DRCVAR_OK;
  int64_t splits = 1;
  if (OT > 0) {
    splits = step_splits > 0 ? step_splits : (kWantedGroups + gx - 1) / gx;
    splits = std::min(splits, std::min(n_steps, int64_t{65535}));
  }
  ClearArgs a{};
  a.steps_per_split = OT > 0 ? (n_steps + splits - 1) / splits : 0;
  if (OT > 0) splits = (n_steps + a.steps_per_split - 1) / a.steps_per_split;  // none empty
  const bool direct = OT > 0 && splits == 1;
  if (!direct) {
    for (int64_t k = 0; k < n_traj; ++k)
      if (hipMemsetAsync(min_clearance_out + k * out_sk, 0xff, static_cast<size_t>(M) * sizeof(double), s) !=
          hipSuccess)
        return DRCVAR_ERR_LAUNCH;
  }
  if (OT > 0) {
    a.ego_sk = ego_sk;
    a.ego_st = ego_st;
    a.nom_so = nom_so;
    a.nom_st = nom_st;
    a.O = n_obstacles;
    a.T = n_steps;
    a.OT = OT;
    a.m_begin = m_begin;
    a.M = M;
    a.p0 = p0;
    a.p1 = p1;
    a.p2 = p2;
    a.R = combined_radius;
    a.RR = combined_radius * combined_radius;
    a.pu = make_philox_uniform(static_cast<uint32_t>(stream_offset),
                               static_cast<uint32_t>(stream_offset >> 32), static_cast<uint32_t>(seed),
                               static_cast<uint32_t>(seed >> 32));
    a.lg = make_log_scale(noise_kind == 1 ? 0.5 : 1.0);
    a.zero_first = zero_first_step != 0;
    a.out_sk = out_sk;
    const dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(splits));
    unsigned long long* hits = reinterpret_cast<unsigned long long*>(step_hits);
    if (noise_kind == 1)
      launch_for_k<true>(static_cast<int>(n_traj), grid, s, ego, nominal, min_clearance_out, hits, a);
    else
      launch_for_k<false>(static_cast<int>(n_traj), grid, s, ego, nominal, min_clearance_out, hits, a);
    if (hipGetLastError() != hipSuccess) return DRCVAR_ERR_LAUNCH;
  }
  if (!direct)
    hipLaunchKernelGGL(clearance_finish_kernel, dim3(static_cast<unsigned>(gx), static_cast<unsigned>(n_traj)),
                       dim3(kBlock), 0, s, min_clearance_out, out_sk, M, combined_radius);
  return hipGetLastError() == hipSuccess ? DRCVAR_OK : DRCVAR_ERR_LAUNCH;
}

extern "C" int drcvar_min_clearance_f64(const double* ego, int64_t n_traj, int64_t ego_sk,
                                        int64_t ego_st, const double* nominal, int64_t n_obstacles,
                                        int64_t n_steps, int64_t nom_so, int64_t nom_st,
                                        int32_t noise_kind, double p0, double p1, double p2,
                                        double combined_radius, int64_t m_begin,
                                        int64_t n_realizations, uint64_t seed, uint64_t stream_offset,
                                        int32_t zero_first_step, double* min_clearance_out,
                                        int64_t out_sk, int64_t* step_hits, void* stream) {
  return drcvar_min_clearance_f64_ex(ego, n_traj, ego_sk, ego_st, nominal, n_obstacles, n_steps,
                                     nom_so, nom_st, noise_kind, p0, p1, p2, combined_radius,
                                     m_begin, n_realizations, seed, stream_offset,
                                     zero_first_step, min_clearance_out, out_sk, step_hits, 0, stream);
}
#endif
