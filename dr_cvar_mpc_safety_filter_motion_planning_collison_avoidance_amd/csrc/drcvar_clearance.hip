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
// partial minimum by an unsigned 64-bit atomic min on the bit pattern of the non-negative d^2
// (the order of non-negative doubles is the order of their bit patterns: exact, independent of
// arrival order), and a finishing launch applies sqrt - R in place.  One split stores directly.
// Both paths take the minimum of the same d^2 values and apply the same sqrt: the same bits.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "drcvar_sampling.h"

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
template <bool kLaplace>
__device__ __forceinline__ void draw_noise(uint64_t g, const ClearArgs& a, const double* s_turn,
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
#pragma unroll
  for (int k = 0; k < K; ++k) mn[k] = inf;
  for (int64_t t = t0; t < t1; ++t) {
    double ex[K], ey[K], mo[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double* e = ego + k * a.ego_sk + t * a.ego_st;
      ex[k] = e[0];
      ey[k] = e[1];
      mo[k] = inf;
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
        mo[k] = min_f64(mo[k], fma(dx, dx, dy * dy));
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      mn[k] = min_f64(mn[k], mo[k]);
      if (hits) {
        const unsigned long long hit = __builtin_amdgcn_ballot_w64(valid && mo[k] < a.RR);
        if (hit != 0 && (threadIdx.x & 63) == 0)
          atomicAdd(hits + k * a.T + t, static_cast<unsigned long long>(__builtin_popcountll(hit)));
      }
    }
  }
  if (!valid) return;
  if (gridDim.y == 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) out[k * a.out_sk + i] = __builtin_sqrt(mn[k]) - a.R;
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k)
      atomicMin(reinterpret_cast<unsigned long long*>(out + k * a.out_sk + i),
                static_cast<unsigned long long>(__double_as_longlong(mn[k])));
  }
}

// The split form's last pass: out[k, i] holds the bit pattern of min d^2 (all-ones where no split
// wrote: the empty O T grid), replaced in place by sqrt - R.
__global__ __launch_bounds__(kBlock) void clearance_finish_kernel(double* out, int64_t out_sk,
                                                                  int64_t M, double R) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= M) return;
  double* p = out + blockIdx.y * out_sk + i;
  const long long bits = __double_as_longlong(*p);
  const double d2 = bits == -1LL ? std::numeric_limits<double>::infinity() : __longlong_as_double(bits);
  *p = __builtin_sqrt(d2) - R;
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

}  // namespace

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
  if (!(p0 == p0) || !(p1 == p1) || !(p2 == p2) || !(combined_radius >= 0.0))
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
