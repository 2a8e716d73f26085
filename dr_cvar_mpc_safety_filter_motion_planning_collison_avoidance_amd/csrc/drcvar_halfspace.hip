// drcvar_halfspace.hip — fused safe-halfspace kernel for MI355X (gfx950, CDNA4) + its C ABI.
//
// One workgroup evaluates one unit = one (obstacle, horizon step): N fp64 samples xi_i in R^2.
// Everything the reference does per unit in core/halfspaces.py:70-194 and core/risk_metrics.py:
// 84-338 happens in ONE pass over HBM (16 B per sample, read once, 16-B/lane coalesced loads):
//
//   1. load the samples into registers (P per thread); one block reduction gives the sums for the
//      mean AND the (pivot-shifted) second moments                        [barrier 1]
//   2. h = (mu - ego)/|mu - ego| ([1,0] if < 1e-10)            core/geometry.py:35-53
//      mean halfspace from the origin                           core/halfspaces.py:84-94
//   3. d_i = h . xi_i                                           core/risk_metrics.py:145,233
//   4. exact (m+1)-th order statistic tau of d, m = floor(alpha*N), sort-free: histogram of d in
//      LDS over [mean_d - 5 sd_d, mean_d + 5 sd_d] (clamped, so every map is monotone in d)
//                                                                         [barrier 2]
//      every wave scans the histogram -> target bucket; when it holds <= kCap samples (the normal
//      case) they are compacted per wave in a fixed order                 [barrier 3]
//      and wave 0 ranks them directly.  Otherwise the bucket is refined (exact min/max, re-histogram;
//      value-linear, then order-preserving integer keys) until <= kCap remain.  Because each map is
//      monotone, a candidate set is always a contiguous run of the sorted order: exact with ties.
//   5. L = tau + sum_{d<tau} (d - tau) / (alpha N)               lower-tail mean = -CVaR_alpha(-d)
//      (= (sum of the m smallest + (alpha N - m) tau) / (alpha N)); the tail sum is accumulated
//      relative to mean_d during the compaction pass, so no further reduction is needed.
//   6. g_cvar = r - delta - L, g* = r - delta + eps/alpha - L, g~ = g* - r, r = R_c |h|
//      (closed-form optimum of the LPs at core/risk_metrics.py:105-125 and :198-213;
//       lambda* = 1/alpha because lambda only enters the budget row and its bound, :110,:122)
//
// Wave reductions use DPP row permutations + readlane (no LDS round trips).  Every reduction and
// the candidate order are fixed, so results are bitwise reproducible run to run.
// No MFMA: ~10 flops per 16-B sample — the kernel is bounded by HBM.
#ifndef DRCVAR_HOST_PLANS_ONLY
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>

#include "drcvar_exchange.h"
#include "drcvar_halfspace.h"

namespace {

// sample load forms (kernel template)
constexpr int kLoadPair = 0, kLoadVec = 1, kLoadNt = 2;
constexpr int64_t kNtBytes = 256ll << 20;  // launches reading more than the MALL use kLoadNt
typedef double dbl2 __attribute__((ext_vector_type(2)));

#ifdef DRCVAR_STAMPS
// diagnostic build only: per-unit shader-clock stamps at phase boundaries (wave 0)
#ifdef DRCVAR_STAMPS_WAVES  // + per-wave stamps (slots 8 + 4j + wave): j = 0, 1 around the load
                            // phase, j = 2 at the end of every wave (which wave exits last)
constexpr int kStampUnits = 16384, kStamps = 24;
#else
constexpr int kStampUnits = 16384, kStamps = 8;
#endif
__device__ unsigned long long g_stamps[kStampUnits * kStamps];
#define DRCVAR_STAMP(k)                                                                       \
  do {                                                                                        \
    const unsigned su_ = blockIdx.y * gridDim.x + blockIdx.x;                                 \
    if (threadIdx.x == 0 && su_ < kStampUnits)                                                \
      g_stamps[su_ * kStamps + (k)] = DRCVAR_STAMP_CLOCK();                                   \
  } while (0)
#ifdef DRCVAR_STAMPS_REALTIME  // 100 MHz clock shared by every XCD: spreads across workgroups
#define DRCVAR_STAMP_CLOCK() __builtin_amdgcn_s_memrealtime()
#else  // shader clock of the workgroup's XCD: phase lengths in cycles
#define DRCVAR_STAMP_CLOCK() __builtin_amdgcn_s_memtime()
#endif
#else
#define DRCVAR_STAMP(k) \
  do {                  \
  } while (0)
#endif
#if defined(DRCVAR_STAMPS) && defined(DRCVAR_STAMPS_WAVES)
#define DRCVAR_STAMP_WAVE(j)                                                                  \
  do {                                                                                        \
    const unsigned su_ = blockIdx.y * gridDim.x + blockIdx.x;                                 \
    if ((threadIdx.x & 63) == 0 && threadIdx.x < 256 && su_ < kStampUnits)                    \
      g_stamps[su_ * kStamps + 8 + 4 * (j) + (threadIdx.x >> 6)] = DRCVAR_STAMP_CLOCK();      \
  } while (0)
#else
#define DRCVAR_STAMP_WAVE(j) \
  do {                       \
  } while (0)
#endif

// the selection toolkit shared with drcvar_sampled.hip: Params, reductions, histogram scan, ranking,
// the exact fallback, the offsets
#include "drcvar_selection.inc"

// KD fp64 and KF fp32 wave sums at once: the same trees as wave_reduce and its fp32 twin (so the
// results are bitwise those of the one-value forms), written stage by stage across the values so
// that the independent chains fill each other's DPP hazard slots (one value at a time, the
// compiler emitted the seven chains back to back: ~750 cycles on the critical path of barrier 1).
template <int CTRL>
__device__ __forceinline__ float mov_dpp_f32(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL, int KD, int KF>
__device__ __forceinline__ void sum_stage(double* v, float* f) {
  double td[KD > 0 ? KD : 1];
  float tf[KF > 0 ? KF : 1];
#pragma unroll
  for (int q = 0; q < KD; ++q) td[q] = dpp_f64<CTRL>(v[q]);
#pragma unroll
  for (int q = 0; q < KF; ++q) tf[q] = mov_dpp_f32<CTRL>(f[q]);
#pragma unroll
  for (int q = 0; q < KD; ++q) v[q] = v[q] + td[q];
#pragma unroll
  for (int q = 0; q < KF; ++q) f[q] = f[q] + tf[q];
}
// (v, f: KD doubles and KF floats in registers — either count may be 0)
// UNIFORM = false skips the last step, the move to SGPRs: the sums stay in VGPRs, where every lane
// holds the same bits already.
template <int KD, int KF, bool UNIFORM = true>
__device__ __forceinline__ void wave_sum_multi(double* v, float* f) {
  sum_stage<kDppQuadXor1, KD, KF>(v, f);
  sum_stage<kDppQuadXor2, KD, KF>(v, f);
  sum_stage<kDppHalfMirror, KD, KF>(v, f);
  sum_stage<kDppMirror, KD, KF>(v, f);
#pragma unroll
  for (int q = 0; q < KD; ++q) v[q] = swap_combine16<OpAdd>(v[q]);
#pragma unroll
  for (int q = 0; q < KF; ++q) {
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_int(f[q]), __float_as_int(f[q]), false, false);
    f[q] = __int_as_float(a[0]) + __int_as_float(a[1]);
  }
#pragma unroll
  for (int q = 0; q < KD; ++q) v[q] = swap_combine32<OpAdd>(v[q]);
#pragma unroll
  for (int q = 0; q < KF; ++q) {
    const auto b = __builtin_amdgcn_permlane32_swap(__float_as_int(f[q]), __float_as_int(f[q]), false, false);
    f[q] = __int_as_float(b[0]) + __int_as_float(b[1]);
  }
  if constexpr (UNIFORM) {
#pragma unroll
    for (int q = 0; q < KD; ++q) v[q] = uniform_f64(v[q]);
#pragma unroll
    for (int q = 0; q < KF; ++q) f[q] = uniform_f32(f[q]);
  }
}

// Workgroup sums of the load phase: KD fp64 values (the mean sums) and KF fp32 values (the
// pivot-shifted second moments, which only position the histogram window).  One barrier.
// `pilot` (optional): the 64-sample pilot published before the barrier — this lane's sample is
// read in the same batch of LDS reads as the partials (read at its first use, after the direction,
// it was a second LDS round trip on the chain to the window pass).
template <int NW, int KD, int KF, bool PILOT = false>
__device__ __forceinline__ void block_sum_moments(double* v, float* f, double* slot_d, float* slot_f,
                                                  const double2* pilot = nullptr,
                                                  double2* pilot_v = nullptr) {
  // Small plans (PILOT) hand the sums over in VGPRs: lane 0 stores its wave's sums from the vector
  // copy, and the workgroup's sums feed the mean and the direction — vector fp64 arithmetic —
  // without a trip through SGPRs on either side of the barrier (those plans run at 59-79 VGPRs;
  // the large ones, at 123-127, keep their uniform values in SGPRs).
  constexpr bool kUniform = !PILOT;
  wave_sum_multi<KD, KF, kUniform>(v, f);
  DRCVAR_STAMP_WAVE(1);  // diagnostic build: this wave's reduction done, before the barrier
  const int lane = threadIdx.x & (kWave - 1);
  if constexpr (NW > 1) {
    const int w = threadIdx.x / kWave;
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < KD; ++q) slot_d[q * NW + w] = v[q];
#pragma unroll
      for (int q = 0; q < KF; ++q) slot_f[q * NW + w] = f[q];
    }
    __syncthreads();
    if constexpr (PILOT) *pilot_v = pilot[lane];
#pragma unroll
    for (int q = 0; q < KD; ++q) v[q] = sum_partials<NW, double, kUniform>(slot_d + q * NW);
#pragma unroll
    for (int q = 0; q < KF; ++q) f[q] = sum_partials<NW, float, kUniform>(slot_f + q * NW);
  } else {
    if constexpr (PILOT) *pilot_v = pilot[lane];  // (one wave: each lane reads back its own store)
  }
  if constexpr (PILOT) asm volatile("" ::"v"(pilot_v->x), "v"(pilot_v->y));
}

// columns 0..2 of the record (the mean halfspace), by one lane
__device__ __forceinline__ void write_mean_halfspace(double* rec, double mux, double muy,
                                                     double rc, int lane) {
  double m0, m1, g_mean;
  mean_halfspace(mux, muy, rc, &m0, &m1, &g_mean);
  if (lane == 0) {
    reinterpret_cast<double2*>(rec)[0] = make_double2(m0, m1);
    rec[DRCVAR_COL_G_MEAN] = g_mean;
  }
}

__device__ __forceinline__ void store_record(double* rec, double m0, double m1, double gm,
                                             double h0, double h1, const Offsets& g) {
  reinterpret_cast<double2*>(rec)[0] = make_double2(m0, m1);
  reinterpret_cast<double2*>(rec)[1] = make_double2(gm, h0);
  reinterpret_cast<double2*>(rec)[2] = make_double2(h1, g.g_cvar);
  reinterpret_cast<double2*>(rec)[3] = make_double2(g.g_star, g.g_tilde);
}

// The peer-push exchange (drcvar_safe_halfspaces_f64_peer, include/drcvar_exchange.h): every
// rank's launch writes each record straight into the exchange region of every rank of the node
// (its own and, over xGMI, the peers' — regions mapped into this process by IPC), at the record's
// global row, in the buffer of this step's parity; drcvar_peer_signal_wait then publishes and
// awaits the generation.  The regions are uncached device memory, and the stores are system-scope
// (write-through) so that no L2 holds a record a peer's later read could miss.
struct PeerArgs {
  double* region[DRCVAR_MAX_PEERS];    // rank j's region (parity 0 rows, parity 1 rows, flags)
  int64_t rows;                        // records per parity buffer (n_ranks * per)
  int64_t row_base;                    // global row of this launch's unit 0
  const unsigned long long* gen;       // this rank's completed-step counter (device)
  int32_t n_ranks;
};

__device__ __forceinline__ void store_sys(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One record to every rank's region: lane j < n_ranks writes rank j's copy (values uniform across
// the wave).  Parity = (completed steps + 1) & 1: the buffer this step fills.
__device__ __forceinline__ void peer_store_record(const PeerArgs& pa, unsigned long long gen,
                                                  int64_t u, int lane, double m0, double m1,
                                                  double gm, double h0, double h1,
                                                  const Offsets& g) {
  if (lane < pa.n_ranks) {
    const int64_t parity = static_cast<int64_t>((gen + 1ull) & 1ull);
    double* r = pa.region[lane] + (parity * pa.rows + pa.row_base + u) * DRCVAR_OUT_WIDTH;
    store_sys(r + 0, m0);
    store_sys(r + 1, m1);
    store_sys(r + 2, gm);
    store_sys(r + 3, h0);
    store_sys(r + 4, h1);
    store_sys(r + 5, g.g_cvar);
    store_sys(r + 6, g.g_star);
    store_sys(r + 7, g.g_tilde);
  }
  // every record store acknowledged (system scope: performed in the destination's memory) before
  // the wave ends, so the publish launch behind this one finds them all in place
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <bool VEC>
__device__ __forceinline__ double project_at(const double* base, int i, int64_t s_samp, double h0,
                                             double h1) {
  const int64_t off = static_cast<int64_t>(i) * s_samp;
  if constexpr (VEC) {
    const double2 v = *reinterpret_cast<const double2*>(base + off);
    return project(h0, h1, v.x, v.y);
  } else {
    return project(h0, h1, base[off], base[off + 1]);
  }
}

// Makes a loaded value available at this point (an empty asm that consumes it): keeps the compiler
// from sinking independent LDS loads past a branch or a wait, so they share one round trip.
__device__ __forceinline__ void lds_values_ready(uint32_t v) { asm volatile("" ::"v"(v)); }
__device__ __forceinline__ void lds_values_ready(double v) { asm volatile("" ::"v"(v)); }

// Offsets from the lower-tail statistics (wave 0, lane 0 writes).  L = tau + dsum / k.
// (The peer form below computes the same values in every lane of wave 0, from lane 0's tau and
// dsum, and writes the whole record — the mean halfspace too — to every rank.)
// r = R_c |h| (risk_metrics.py:293, :234), computed by the caller as soon as h is known.
template <int NW>
__device__ __forceinline__ void finish_offsets(double* rec, const Params& prm, double r, double h0,
                                               double h1, double tau, double dsum, double mux,
                                               double muy, int lane) {
  if (lane == 0) {
    const Offsets g = offsets_from_tail(prm, r, tau, dsum);
    if constexpr (NW == 1) {
      double m0, m1, g_mean;
      mean_halfspace(mux, muy, prm.rc, &m0, &m1, &g_mean);
      store_record(rec, m0, m1, g_mean, h0, h1, g);
    } else {  // columns 0..2 are written by wave 1
      reinterpret_cast<double*>(rec)[DRCVAR_COL_H0] = h0;
      reinterpret_cast<double2*>(rec)[2] = make_double2(h1, g.g_cvar);
      reinterpret_cast<double2*>(rec)[3] = make_double2(g.g_star, g.g_tilde);
    }
  }
}

__device__ __forceinline__ void finish_offsets_peer(const PeerArgs& pa, unsigned long long gen,
                                                    int64_t u, const Params& prm, double r,
                                                    double h0, double h1, double tau, double dsum,
                                                    double mux, double muy, int lane) {
  tau = readlane_f64(tau, 0);
  dsum = readlane_f64(dsum, 0);
  const Offsets g = offsets_from_tail(prm, r, tau, dsum);
  double m0, m1, g_mean;
  mean_halfspace(mux, muy, prm.rc, &m0, &m1, &g_mean);
  peer_store_record(pa, gen, u, lane, m0, m1, g_mean, h0, h1, g);
}


// ---------------------------------------------------------------------------------------------
// the fused kernel
//   BLOCK    threads per unit (one workgroup per unit)
//   P        samples held per thread (N <= BLOCK * P)
//   LOG_NB   log2 of histogram bins
//   LOAD     kLoadPair: two 8-B loads per sample; kLoadVec: every (x, y) pair is 16-B aligned ->
//            one 16-B load per sample; kLoadNt: the same, nontemporal (launches larger than the
//            256 MB Infinity Cache, whose samples are streamed exactly once)
//   GIVEN_H  `dir` holds h per unit (cvar_halfspace / dr_cvar_halfspace) instead of ego per step
// ---------------------------------------------------------------------------------------------
//   PEER     the peer-push exchange form: records go to every rank's exchange region (PeerArgs)
//            instead of `out`
//   FULL     small plans (P <= 8) only: the host saw N > BLOCK * (P - 1), so rows 0 .. P-2 hold a
//            sample in every thread and carry no `i < n` selects; the last row keeps them
//   LONE     small plans (P <= 8), not the peer or the nontemporal form: the host saw a grid of no
//            more workgroups than the device has CUs, so this workgroup has its CU to itself and
//            only its own chain counts — the candidate pass stores under a narrowed exec mask
//            instead of behind a branch (append_candidate_masked).  On a full CU the branch is
//            the cheaper form (1-3 % on C3 replicated to 2 GB), so larger grids keep it.
template <int BLOCK, int P, int LOG_NB, int LOAD, bool GIVEN_H, bool PEER, bool FULL,
          bool LONE = false>
__global__ void __launch_bounds__(BLOCK)
safe_halfspace_kernel(const double* __restrict__ samples, int64_t n_steps, int n,
                      int64_t s_obs, int64_t s_step, int64_t s_samp,
                      const double* __restrict__ dir, int64_t dir_s_obs, int64_t dir_s_step,
                      Params prm, double* __restrict__ out, int32_t* __restrict__ status,
                      PeerArgs peer) {
  constexpr int NW = BLOCK / kWave;
  constexpr int NB = 1 << LOG_NB;
  __shared__ uint32_t hist[hist_words<NB>()];
  __shared__ double cand[NW * kCap];
  __shared__ double lane_tail[P <= 8 ? BLOCK : 1];
  __shared__ uint32_t wcount[NW];
  __shared__ uint32_t wbelow_sh[NW];
  // Small plans (the latency-bound ones) place the histogram window from a 64-sample pilot after
  // barrier 1 — the variance of the projections themselves, one two-value wave reduction —
  // instead of reducing five row-0 second moments across the workgroup before it: per-wave stamps
  // (-DDRCVAR_STAMPS_WAVES) showed the seven-value reduction at ~1 000 cycles of one wave's issue
  // on the chain to barrier 1.  Large plans (bandwidth-bound) keep the row-0 moments, whose larger
  // subsample gives their narrower windows (0.25 sd at N = 10 000) more margin.
  constexpr bool kPilot = P <= 8;
  __shared__ double2 pilot[kPilot ? kWave : 1];
  __shared__ double red_mom[2 * NW];
  __shared__ float red_mom0[5 * NW];
  __shared__ double red_rng[2 * NW];
  __shared__ double red_tail[NW];

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid / kWave;
  // grid (n_steps, n_obstacles): no integer division ahead of the sample loads (the host splits
  // launches of more than 65535 obstacles)
  const int64_t o = blockIdx.y, t = blockIdx.x;
  const int64_t u = o * n_steps + t;
  const double* base = samples + o * s_obs + t * s_step;
  double* rec = out + u * DRCVAR_OUT_WIDTH;

  DRCVAR_STAMP(0);

  // ---- 1. load + moments ----------------------------------------------------------------
  // Branch-free: idle slots of the last row re-load sample n-1 and contribute zeros.  Offsets:
  // one 64-bit product for the thread's first sample, then a uniform step per row (the clamp is a
  // select, not a product per sample: the per-sample quarter-rate multiplies sat before the
  // loads were issued).
  double x[P], y[P];
  const int64_t off0 = static_cast<int64_t>(tid) * s_samp;
  const int64_t row_step = static_cast<int64_t>(BLOCK) * s_samp;
  const int64_t off_last = static_cast<int64_t>(n - 1) * s_samp;
  // does this thread's slot of row j hold a sample?  (a constant for the rows known full)
  const auto in_row = [&](int j) { return (FULL && j < P - 1) || tid + j * BLOCK < n; };
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int64_t off = in_row(j) ? off0 + j * row_step : off_last;
    if constexpr (LOAD == kLoadNt) {  // streamed once: keep it out of L2 / MALL
      const dbl2 v = __builtin_nontemporal_load(reinterpret_cast<const dbl2*>(base + off));
      x[j] = v.x;
      y[j] = v.y;
    } else if constexpr (LOAD == kLoadVec) {
      const double2 v = *reinterpret_cast<const double2*>(base + off);
      x[j] = v.x;
      y[j] = v.y;
    } else {
      x[j] = base[off];
      y[j] = base[off + 1];
    }
  }
  // The unit's direction input and the early scalars are fetched while the 16-B sample loads
  // are in flight (otherwise the compiler sinks these scalar loads to their first use, after
  // barrier 1, and their latency lands on the critical path).
  // The pivot of the row-0 moments (the unit's first sample, a uniform scalar load) is issued in
  // the same batch: loaded after the wait for the direction input, it put a second scalar-memory
  // round trip in series on the way to the first moment sums.
  const double* dp = dir + o * dir_s_obs + t * dir_s_step;
  const double e0 = dp[0], e1 = dp[1];
  double px = 0.0, py = 0.0;  // row-0 moments' pivot: the unit's first sample
  if constexpr (!kPilot) {
    px = base[0];
    py = base[1];
  }
  const double inv_n = prm.inv_n, inv_n0 = prm.inv_n0, deg_sq = prm.degenerate_sq;
  const double z_lo = prm.z_lo, hist_scale = prm.hist_scale;
  // inv_k too: first used by the offsets, it was fetched only after the histogram scan, and the
  // candidate pass waited for that scalar load (its lgkm wait also covers the kernarg fetch)
  const double inv_k = prm.inv_k;
  asm volatile("" ::"s"(e0), "s"(e1), "s"(px), "s"(py), "s"(inv_n), "s"(inv_n0), "s"(deg_sq),
               "s"(z_lo), "s"(hist_scale), "s"(inv_k), "s"(status));
  unsigned long long gen = 0;  // the peer form's completed-step counter (parity of the buffer)
  if constexpr (PEER) gen = *peer.gen;
  // the histogram is cleared while the sample loads are in flight (barrier 1 orders it before
  // the first atomic)
#pragma unroll
  for (int b = tid; b < hist_words<NB>(); b += BLOCK) hist[b] = 0u;
  // Sums for the mean over every sample (plain sums, as np.mean, in fp64); second moments over
  // row 0 only (the first BLOCK samples), shifted by the unit's first sample and summed in fp32 —
  // they merely position the fast-path window, so a subsample at low precision is enough: an
  // inaccurate window can only cost speed (the exact fallback), never exactness.
  double mom[2] = {0.0, 0.0};               // Sx Sy
  float mom0[5] = {0.f, 0.f, 0.f, 0.f, 0.f};  // row 0, pivot-shifted: Sa Sb Saa Sbb Sab
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const bool valid = in_row(j);
    const double a = valid ? x[j] : 0.0, b = valid ? y[j] : 0.0;
    mom[0] += a;
    mom[1] += b;
    if (!kPilot && j == 0) {
      const float fa = valid ? static_cast<float>(x[0] - px) : 0.f;
      const float fb = valid ? static_cast<float>(y[0] - py) : 0.f;
      mom0[0] = fa;
      mom0[1] = fb;
      mom0[2] = fa * fa;
      mom0[3] = fb * fb;
      mom0[4] = fa * fb;
    }
  }
  if (kPilot && wave == 0) pilot[lane] = make_double2(x[0], y[0]);  // samples 0..63 (lane < n)
  DRCVAR_STAMP(1);
  DRCVAR_STAMP_WAVE(0);  // diagnostic build: this wave's samples summed (its loads done)
  double2 pv = make_double2(0.0, 0.0);  // this lane's pilot sample (small plans)
  if constexpr (kPilot)
    block_sum_moments<NW, 2, 0, true>(mom, mom0, red_mom, red_mom0, pilot, &pv);  // [barrier 1]
  else
    block_sum_moments<NW, 2, 5>(mom, mom0, red_mom, red_mom0);           // [barrier 1]
  DRCVAR_STAMP(2);
  const double mux = mom[0] * inv_n, muy = mom[1] * inv_n;
  // any non-finite sample makes a sum non-finite (so do sums that overflow): solver failure
  const bool bad = !(std::isfinite(mom[0]) && std::isfinite(mom[1]));

  // ---- 2. direction ----------------------------------------------------------------------
  double h0, h1;
  if constexpr (GIVEN_H) {
    h0 = e0;
    h1 = e1;
  } else {
    separating_direction<rsqrt_nr>(mux, muy, e0, e1, deg_sq, &h0, &h1);
  }
  if (bad || prm.unbounded) {  // solver failure, risk_metrics.py:298-303,334-338
    if constexpr (PEER) {
      if (wave == 0) {
        const double r = prm.rc * norm_h(h0, h1);  // R_c |h|
        double m0, m1, g_mean;
        mean_halfspace(mux, muy, prm.rc, &m0, &m1, &g_mean);
        peer_store_record(peer, gen, u, lane, m0, m1, g_mean, h0, h1, failure_offsets(r));
        if (status && lane == 0) status[u] = failure_status(bad, prm);
      }
      return;
    }
    if (tid == 0) {
      const double r = prm.rc * norm_h(h0, h1);  // R_c |h|
      double m0, m1, g_mean;
      mean_halfspace(mux, muy, prm.rc, &m0, &m1, &g_mean);
      store_record(rec, m0, m1, g_mean, h0, h1, failure_offsets(r));
      if (status) status[u] = failure_status(bad, prm);
    }
    return;  // uniform across the workgroup
  }

  // ---- 3. projections; window histogram around the estimated quantile ------------------------
  double d[P];
#pragma unroll
  for (int j = 0; j < P; ++j)  // +inf padding: never below, inside or a candidate
    d[j] = in_row(j) ? project(h0, h1, x[j], y[j]) : INFINITY;
  const double mu_d = h0 * mux + h1 * muy;
  double var_d;
  if constexpr (kPilot) {  // variance of the pilot's projections about the exact mean, in fp32
    float fm[2];
    fm[0] = lane < n ? static_cast<float>(project(h0, h1, pv.x, pv.y) - mu_d) : 0.f;
    fm[1] = fm[0] * fm[0];
    wave_sum_multi<0, 2>(nullptr, fm);
    const double m1 = fm[0] * inv_n0;
    var_d = fm[1] * inv_n0 - m1 * m1;
  } else {
    const double ma0 = mom0[0] * inv_n0, mb0 = mom0[1] * inv_n0;  // row-0 covariance
    const double cxx = mom0[2] * inv_n0 - ma0 * ma0, cyy = mom0[3] * inv_n0 - mb0 * mb0;
    const double cxy = mom0[4] * inv_n0 - ma0 * mb0;
    var_d = h0 * h0 * cxx + 2.0 * h0 * h1 * cxy + h1 * h1 * cyy;
  }
  // window [wlo, wlo + 2 window_sd sd_d), wlo = mean_d + (z_alpha - window_sd) sd_d; only
  // samples inside it are histogrammed (LDS atomics), samples below it are counted with ballots.
  // Any positive scale keeps the map monotone, so the approximate reciprocal sqrt is exact enough.
  const double inv_sd = rsqrt_nr(var_d);
  const double sd_d = var_d * inv_sd;
  const double wlo = fma(z_lo, sd_d, mu_d);
  const double scale = prm.hist_scale * inv_sd;
  const LinearMap map{scale, -wlo * scale};
  const uint32_t rank = prm.rank;
  bool fast = var_d > 0.0 && std::isfinite(map.scale) && std::isfinite(map.off) && map.scale > 0.0;
  constexpr double kNB = static_cast<double>(NB);
  uint32_t rr = rank, c = 0;
  int bin = 0;
  // per-sample bucket codes, two 16-bit codes per register: the bin inside the window, 0xFFFF
  // outside it (the sum of samples below the window is taken in this pass)
  constexpr int PC = (P + 1) / 2;
  uint32_t code[PC];
  double sq = 0.0;  // sum over samples below the target bucket of (d - mu_d)
  if (fast) {
    uint32_t wbelow = 0;  // samples of this wave below the window (wave-uniform)
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const double v = d[j];
      const double tv = map(v);
      const bool low = tv < 0.0;
      wbelow += static_cast<uint32_t>(__popcll(__ballot(low)));
      sq += low ? v - mu_d : 0.0;
      const bool inw = !low && tv < kNB;
      const int b = inw ? static_cast<int>(tv) : 0;  // 0 <= b <= NB - 1 inside the window
      if (inw) atomicAdd(&hist[hist_slot<NB>(b)], 1u);
      const uint32_t cj = inw ? static_cast<uint32_t>(b) : 0xFFFFu;
      if (j % 2 == 0) code[j / 2] = cj;
      else code[j / 2] |= cj << 16;
    }
    if (lane == 0) wbelow_sh[wave] = wbelow;
    DRCVAR_STAMP(3);
    __syncthreads();                                                      // [barrier 2]
    uint32_t hb[NB / kWave];  // this lane's bins, read together with the per-wave counts
    load_bins<NB>(hist, lane, hb);
    uint32_t below = 0;  // all samples below the window
#pragma unroll
    for (int w = 0; w < NW; ++w) below += wbelow_sh[w];
    // the bins are wanted only when the target lies in the window (a branch on `below`): without
    // this the compiler issued their loads inside the branch, a second LDS round trip after the
    // wait for the counts
#pragma unroll
    for (int b = 0; b < NB / kWave; ++b) lds_values_ready(hb[b]);
    if (rank >= below) {
      const ScanResult sr = scan_loaded_bins<NB>(hb, rank - below, lane);  // every wave, same result
      bin = sr.bin;
      rr = rank - below - sr.below;
      c = sr.cnt;
      fast = sr.found && c <= kCap;
    } else {
      fast = false;  // tau lies below the window (far from Gaussian): exact fallback
    }
    DRCVAR_STAMP(4);
  }

  // ---- 4. candidates of the target bucket + tail sum below them -----------------------------
  double tau, dsum;  // dsum = sum_{d<tau} (d - tau)
  double rch;        // R_c |h| (risk_metrics.py:293, :234), wave 0
  if (fast) [[likely]] {
    uint32_t wbase = 0;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const uint32_t ubin = static_cast<uint32_t>(bin);
    // The express finish: of a bucket of c <= 64 / NW candidates (every wave knows c from the
    // scan) no wave holds more than E = 64 / NW, so wave w writes its candidates to the segment
    // cand[w * E ..) instead of its region cand[w * kCap ..): all of the unit's candidates lie in
    // cand[0 .. 64), in the ranking's order, and wave 0 reads them — one per lane — in the same
    // batch as the counts and the tail partials: no slot computation and no second, dependent LDS
    // round trip ahead of the ranking.  Larger buckets keep the regions (a uniform branch on c).
    const bool express = c <= static_cast<uint32_t>(kWave / NW);
    double* const cregion = cand + wave * (express ? kWave / NW : kCap);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const uint32_t cj = (code[j / 2] >> (16 * (j % 2))) & 0xFFFFu;
      sq += cj < ubin ? d[j] - mu_d : 0.0;
      if constexpr (LONE) append_candidate_masked(cregion, wbase, cj == ubin, d[j], lt_mask);
      else append_candidate(cregion, wbase, cj == ubin, d[j], lt_mask);
    }
    if constexpr (kPilot) {
      // small plans: this lane's tail partial goes to LDS unreduced; wave 0 reduces the four waves'
      // partials once after barrier 3, beside the ranking's LDS reads, instead of every wave
      // reducing its own ahead of the barrier
      lane_tail[tid] = sq;
      if (lane == 0) wcount[wave] = wbase;
      if constexpr (LONE) lds_masked_wait();  // the masked candidate stores, ahead of barrier 3
    } else {
      sq = wave_reduce<OpAdd>(sq);
      if (lane == 0) {
        red_tail[wave] = sq;
        wcount[wave] = wbase;
      }
    }
    DRCVAR_STAMP(5);
    __syncthreads();                                                      // [barrier 3]
    DRCVAR_STAMP(6);
    if (wave != 0) {
      if (!PEER && wave == 1) write_mean_halfspace(rec, mux, muy, prm.rc, lane);
      DRCVAR_STAMP_WAVE(2);  // diagnostic build: this wave's end
      return;
    }
    // One batch of LDS reads: the per-wave candidate counts (cw: lane w < NW holds wave w's, the
    // region ranking's input — read by every lane, lane l wave l % NW's, which needs no exec mask;
    // cx: lane l holds the count of the wave whose segment l lies in, the express ranking's
    // validity test), this lane's candidate of the segment layout (unused, any value, on a larger
    // bucket) and the tail partials.
    const uint32_t cw = wcount[lane & (NW - 1)];
    const uint32_t cx = wcount[lane / (kWave / NW)];
    const double mine = cand[lane];
    double s_below;
    [[maybe_unused]] double tail_lane = 0.0;  // small plans: this lane's sum of the waves' tail partials
    if constexpr (kPilot) {
      double tl[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) tl[w] = lane_tail[w * kWave + lane];
      // R_c |h| while the reads are in flight: off the histogram's critical path, and off the
      // finish's (computed after the tail's reduction, it stood in series with the ranking)
      rch = prm.rc * norm_h(h0, h1);
      lds_values_ready(rch);
      lds_values_ready(cw);
      lds_values_ready(cx);
      lds_values_ready(mine);
      double t = tl[0];
#pragma unroll
      for (int w = 1; w < NW; ++w) t += tl[w];
      tail_lane = t;  // reduced over the wave beside the ranking's first candidate, below
    } else {
      s_below = sum_partials<NW>(red_tail);
      lds_values_ready(cw);
      lds_values_ready(cx);
      lds_values_ready(mine);
      rch = prm.rc * norm_h(h0, h1);  // R_c |h|: off the histogram's critical path
    }
    double s_cand;
    if constexpr (kPilot) {
      // the tail's wave reduction in one basic block with the ranking's first candidate
      if (express) [[likely]] {
        tau = rank_candidates_express_tail<NW>(mine, cx, rr, lane, tail_lane, &s_below, &s_cand);
      } else {
        s_below = wave_reduce<OpAdd>(tail_lane);
        tau = rank_candidates<NW>(cand, cw, c, rr, lane, &s_cand);
      }
    } else if (express) [[likely]]
      tau = rank_candidates_express<NW>(mine, cx, rr, lane, &s_cand);
    else
      tau = rank_candidates<NW>(cand, cw, c, rr, lane, &s_cand);
    dsum = (s_below - static_cast<double>(rank - rr) * (tau - mu_d)) + s_cand;
  } else [[unlikely]] {
    // No spread in the moments: the noise-free step 0 of every obstacle (simulation/obstacles.py:63)
    // has all samples equal — settled from the registers by one min/max reduction (tau = the
    // common value, no tail below it) instead of the re-reading fallback, which costs two passes
    // over memory and four barriers and made these units the slowest of a launch.
    // Small plans only: on the 20-sample plan the extra live range costs the second workgroup
    // per CU (127 -> 130 VGPRs), and a C5 launch is bandwidth-bound, not set by its slowest unit.
    bool settled = false;
    if (P <= 8 && !(var_d > 0.0)) {  // uniform
      double lo[1] = {INFINITY}, hi[1] = {-INFINITY};
#pragma unroll
      for (int j = 0; j < P; ++j) {
        if (tid + j * BLOCK < n) {
          lo[0] = fmin(lo[0], d[j]);
          hi[0] = fmax(hi[0], d[j]);
        }
      }
      block_reduce<OpMin, NW, 1>(lo, red_rng);
      block_reduce<OpMax, NW, 1>(hi, red_rng + NW);
      if (lo[0] == hi[0]) {  // uniform (the reductions end with identical values in every lane)
        tau = lo[0];
        dsum = 0.0;
        settled = true;
      }
    }
    if (!settled) {
      const auto proj = [&](int i) { return project_at<LOAD != kLoadPair>(base, i, s_samp, h0, h1); };
      select_exact<BLOCK, LOG_NB>(memory_source<BLOCK>(proj, n), mu_d, rank, hist, cand, wcount,
                                  red_rng, red_tail, &tau, &dsum);
    }
    if (wave != 0) {
      if (!PEER && wave == 1) write_mean_halfspace(rec, mux, muy, prm.rc, lane);
      DRCVAR_STAMP_WAVE(2);  // diagnostic build: this wave's end
      return;
    }
    rch = prm.rc * norm_h(h0, h1);
  }

  // ---- 5. offsets (wave 0) -------------------------------------------------------------------
  if constexpr (PEER)
    finish_offsets_peer(peer, gen, u, prm, rch, h0, h1, tau, dsum, mux, muy, lane);
  else
    finish_offsets<NW>(rec, prm, rch, h0, h1, tau, dsum, mux, muy, lane);
  if (status && lane == 0) status[u] = failure_status(false, prm);
  DRCVAR_STAMP(7);
  DRCVAR_STAMP_WAVE(2);
}


// ---------------------------------------------------------------------------------------------
// streaming variant for N > DRCVAR_MAX_SAMPLES: nothing is held in registers — the mean is a
// strided pass over the unit's samples and the order statistic comes from select_exact's
// histogram refinement over re-reads (min/max pass, ~1 histogram pass per factor 10^3 of
// N, a candidate pass).  Any N up to 2^31 - 1; ~4 reads of the unit instead of 1.
// ---------------------------------------------------------------------------------------------
constexpr int kStreamBlock = 1024;
constexpr int kStreamLogNB = 10;

template <bool VEC, bool GIVEN_H>
__global__ void __launch_bounds__(kStreamBlock)
safe_halfspace_stream_kernel(const double* __restrict__ samples, int64_t n_steps, int n,
                             int64_t s_obs, int64_t s_step, int64_t s_samp,
                             const double* __restrict__ dir, int64_t dir_s_obs,
                             int64_t dir_s_step, Params prm, double* __restrict__ out,
                             int32_t* __restrict__ status) {
  constexpr int BLOCK = kStreamBlock;
  constexpr int NW = BLOCK / kWave;
  constexpr int NB = 1 << kStreamLogNB;
  __shared__ uint32_t hist[hist_words<NB>()];
  __shared__ double cand[NW * kCap];
  __shared__ uint32_t wcount[NW];
  __shared__ double red_mom[2 * NW];
  __shared__ double red_rng[2 * NW];
  __shared__ double red_tail[NW];
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid / kWave;
  const int64_t u = blockIdx.x;
  const int64_t o = u / n_steps;
  const int64_t t = u - o * n_steps;
  const double* base = samples + o * s_obs + t * s_step;
  double* rec = out + u * DRCVAR_OUT_WIDTH;
  double mom[2] = {0.0, 0.0};
  for (int i = tid; i < n; i += BLOCK) {
    const double* pt = base + static_cast<int64_t>(i) * s_samp;
    if constexpr (VEC) {
      const double2 v = *reinterpret_cast<const double2*>(pt);
      mom[0] += v.x;
      mom[1] += v.y;
    } else {
      mom[0] += pt[0];
      mom[1] += pt[1];
    }
  }
  block_reduce<OpAdd, NW, 2>(mom, red_mom);
  const double mux = mom[0] * prm.inv_n, muy = mom[1] * prm.inv_n;
  const bool bad = !(std::isfinite(mom[0]) && std::isfinite(mom[1]));
  const double* dp = dir + o * dir_s_obs + t * dir_s_step;
  double h0, h1;
  if constexpr (GIVEN_H) {
    h0 = dp[0];
    h1 = dp[1];
  } else {
    separating_direction<rsqrt_nr>(mux, muy, dp[0], dp[1], prm.degenerate_sq, &h0, &h1);
  }
  const double rch = prm.rc * norm_h(h0, h1);  // R_c |h|
  if (bad || prm.unbounded) {
    if (tid == 0) {
      double m0, m1, g_mean;
      mean_halfspace(mux, muy, prm.rc, &m0, &m1, &g_mean);
      store_record(rec, m0, m1, g_mean, h0, h1, failure_offsets(rch));
      if (status) status[u] = failure_status(bad, prm);
    }
    return;
  }
  const double mu_d = h0 * mux + h1 * muy;
  double tau, dsum;
  const auto proj = [&](int i) { return project_at<VEC>(base, i, s_samp, h0, h1); };
  select_exact<BLOCK, kStreamLogNB>(memory_source<BLOCK>(proj, n), mu_d, prm.rank, hist, cand,
                                    wcount, red_rng, red_tail, &tau, &dsum);
  if (wave != 0) {
    if (wave == 1) write_mean_halfspace(rec, mux, muy, prm.rc, lane);
    return;
  }
  finish_offsets<NW>(rec, prm, rch, h0, h1, tau, dsum, mux, muy, lane);
  if (status && lane == 0) status[u] = failure_status(false, prm);
}

// ---------------------------------------------------------------------------------------------
// launch plans
// ---------------------------------------------------------------------------------------------
#endif  // !DRCVAR_HOST_PLANS_ONLY
// The host's choice of launch plan and kernel form: plain C++, no HIP, nothing but <cstdint> and
// drcvar_halfspace.h before it.  With -DDRCVAR_HOST_PLANS_ONLY this section is all of the file that
// is compiled: tests/test_halfspace_form_host.py includes the file that way into a stand-alone
// program of the host compiler and checks the rule without a GPU.
struct Plan {
  int block, per, log_nb;
  bool automatic;  // part of the default chain (smallest automatic plan with block*per >= N)
};
constexpr Plan kPlans[] = {
    {64, 2, 7, true},       // N <=   128
    {128, 4, 8, true},      // N <=   512
    {256, 4, 9, true},      // N <=  1024
    {256, 8, 10, true},     // N <=  2048
    {256, 16, 10, true},    // N <=  4096
    {256, 20, 10, true},    // N <=  5120   (C4 N = 5000: 27.3 us vs 38.9 us on 512 x 16)
    {512, 16, 10, true},    // N <=  8192   (2 workgroups per CU)
    {512, 20, 10, true},    // N <= 10240   (2 workgroups per CU)
    {1024, 12, 10, true},   // N <= 12288
    {1024, 16, 10, true},   // N <= 16384
    // alternative geometries, selectable through drcvar_safe_halfspaces_f64_ex (tuning)
    {64, 16, 9, false},
    {128, 8, 9, false},
    {512, 2, 9, false},
    {1024, 10, 10, false},
};
constexpr int kNumPlans = sizeof(kPlans) / sizeof(kPlans[0]);

inline int pick_plan(int64_t n, int threads, int per) {
  for (int p = 0; p < kNumPlans; ++p) {
    const Plan& pl = kPlans[p];
    if (n > static_cast<int64_t>(pl.block) * pl.per) continue;
    if (threads == 0 && per == 0) {
      if (pl.automatic) return p;
    } else if (pl.block == threads && pl.per == per) {
      return p;
    }
  }
  return -1;
}

// The two forms of the kernel.  LONE: the candidate pass stores under a narrowed exec mask
// instead of behind a branch — faster for a workgroup that has its CU to itself, slower where the
// CUs are full (docs/lab_notebook.md section 4).  The whole rule is here: the plans that have the
// form (those holding at most kLoneMaxPer samples per thread, not the peer form), and the launches
// that take it (no more units than the device has CUs, so no CU gets a second workgroup).
constexpr int kFormShared = 0, kFormLone = 1;
constexpr int kLoneMaxPer = 8;
constexpr bool lone_capable(int per, bool peer) { return per <= kLoneMaxPer && !peer; }
constexpr bool lone_form(int per, bool peer, int64_t units, int cu_count) {
  return lone_capable(per, peer) && units >= 1 && units <= cu_count;
}

// The form an automatic, non-peer launch of n_units units of n_samples samples takes on a device
// with cu_count CUs (what dispatch computes, with the argument checks of drcvar_launch_plan).
inline int halfspace_form(int64_t n_samples, int64_t n_units, int32_t cu_count, int32_t* form) {
  if (n_samples < 1 || n_units < 0 || cu_count < 1 || !form) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (n_samples > DRCVAR_MAX_SAMPLES) {  // the streaming kernel has one form
    if (n_samples > DRCVAR_MAX_SAMPLES_STREAM) return DRCVAR_ERR_UNSUPPORTED;
    *form = kFormShared;
    return DRCVAR_OK;
  }
  const int p = pick_plan(n_samples, 0, 0);
  if (p < 0) return DRCVAR_ERR_UNSUPPORTED;
  *form = lone_form(kPlans[p].per, false, n_units, cu_count) ? kFormLone : kFormShared;
  return DRCVAR_OK;
}
#ifndef DRCVAR_HOST_PLANS_ONLY

struct Launch {
  const double* samples;
  int64_t units, n_steps, n, s_obs, s_step, s_samp;
  const double* dir;
  int64_t dir_s_obs, dir_s_step;
  Params prm;
  double* out;
  int32_t* status;  // [units] or null
  hipStream_t stream;
  PeerArgs peer;    // the peer form only
  bool lone;        // no more units than the device has CUs (dispatch)
};

// CUs of the calling thread's current device, asked once per device and cached: two attribute
// queries, no allocation, no synchronisation, nothing a stream capture forbids — a process whose
// first launch is captured into a graph gets its answer the same way.  The launch is assumed to
// run on the current device (bench.py, the tests and the drop-in layer all make the device of
// their tensors current); a stream of another device would only have its form chosen by this
// device's CU count, never get other results.  0 (never the LONE
// form) if the runtime does not answer.
constexpr int kMaxDevices = 64;
std::atomic<int> g_cu_count[kMaxDevices];
int device_cu_count() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 0;
  int cus = g_cu_count[dev].load(std::memory_order_relaxed);
  if (cus == 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus < 0)
      cus = 0;
    g_cu_count[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}

// grid (n_steps, obstacles), at most kMaxGridY obstacles per launch (the y-dimension limit):
// larger batches are split into obstacle chunks on the host
constexpr int64_t kMaxGridY = 65535;

template <int BLOCK, int P, int LOG_NB, int LOAD, bool GIVEN_H, bool PEER, bool FULL,
          bool LONE = false>
int launch_form(const Launch& L) {
  const int64_t n_obs = L.units / L.n_steps;
  const size_t dyn = 0;
  for (int64_t o0 = 0; o0 < n_obs; o0 += kMaxGridY) {
    const int64_t chunk = n_obs - o0 < kMaxGridY ? n_obs - o0 : kMaxGridY;
    PeerArgs pa = L.peer;
    pa.row_base += o0 * L.n_steps;
    hipLaunchKernelGGL((safe_halfspace_kernel<BLOCK, P, LOG_NB, LOAD, GIVEN_H, PEER, FULL, LONE>),
                       dim3(static_cast<unsigned>(L.n_steps), static_cast<unsigned>(chunk)),
                       dim3(BLOCK), dyn, L.stream, L.samples + o0 * L.s_obs, L.n_steps,
                       static_cast<int>(L.n), L.s_obs, L.s_step, L.s_samp,
                       L.dir + o0 * L.dir_s_obs, L.dir_s_obs, L.dir_s_step, L.prm,
                       L.out + o0 * L.n_steps * DRCVAR_OUT_WIDTH,
                       L.status ? L.status + o0 * L.n_steps : nullptr, pa);
  }
  return DRCVAR_OK;
}

// Small plans whose N fills every row but the last run the form without those rows' `i < n`
// selects; any other N (an explicit geometry far larger than N included) the predicated form.
// Either in the LONE form when dispatch found the launch to meet lone_form
// (above); a launch of that size is far below the nontemporal form's 256 MB.
template <int BLOCK, int P, int LOG_NB, int LOAD, bool GIVEN_H, bool PEER>
int launch_rows(const Launch& L) {
  if constexpr (P <= 8) {
    const bool full = L.n > static_cast<int64_t>(BLOCK) * (P - 1);
    if constexpr (lone_capable(P, PEER) && LOAD != kLoadNt) {
      if (L.lone) {
        return full ? launch_form<BLOCK, P, LOG_NB, LOAD, GIVEN_H, PEER, true, true>(L)
                    : launch_form<BLOCK, P, LOG_NB, LOAD, GIVEN_H, PEER, false, true>(L);
      }
    }
    if (full) return launch_form<BLOCK, P, LOG_NB, LOAD, GIVEN_H, PEER, true>(L);
  }
  return launch_form<BLOCK, P, LOG_NB, LOAD, GIVEN_H, PEER, false>(L);
}

template <int BLOCK, int P, int LOG_NB, bool GIVEN_H, bool PEER>
int launch_plan(Launch L, bool vec) {
  const int64_t sub = P <= 8 ? kWave : BLOCK;  // the window's subsample: pilot or row 0 (kernel)
  L.prm.inv_n0 = 1.0 / static_cast<double>(L.n < sub ? L.n : sub);
  L.prm.hist_scale = static_cast<double>(1 << LOG_NB) / (2.0 * L.prm.window_sd);
  // measured on C5 (2.05 GB): nontemporal 16-B loads 0.746 of HBM peak vs 0.715; on C3 (3.2 MB,
  // cache-resident across steps) they cost 3 %, so only launches larger than the MALL use them
  const bool nt = vec && L.units * L.n * 16 > kNtBytes;
  if (nt) return launch_rows<BLOCK, P, LOG_NB, kLoadNt, GIVEN_H, PEER>(L);
  if (vec) return launch_rows<BLOCK, P, LOG_NB, kLoadVec, GIVEN_H, PEER>(L);
  if constexpr (PEER) return DRCVAR_ERR_UNSUPPORTED;  // the peer form reads packed 16-B samples
  else return launch_rows<BLOCK, P, LOG_NB, kLoadPair, GIVEN_H, false>(L);
}

template <bool GIVEN_H>
void launch_stream(const Launch& L, bool vec) {
  const dim3 grid(static_cast<unsigned>(L.units)), block(kStreamBlock);
  if (vec) {
    hipLaunchKernelGGL((safe_halfspace_stream_kernel<true, GIVEN_H>), grid, block, 0, L.stream,
                       L.samples, L.n_steps, static_cast<int>(L.n), L.s_obs, L.s_step, L.s_samp,
                       L.dir, L.dir_s_obs, L.dir_s_step, L.prm, L.out, L.status);
  } else {
    hipLaunchKernelGGL((safe_halfspace_stream_kernel<false, GIVEN_H>), grid, block, 0, L.stream,
                       L.samples, L.n_steps, static_cast<int>(L.n), L.s_obs, L.s_step, L.s_samp,
                       L.dir, L.dir_s_obs, L.dir_s_step, L.prm, L.out, L.status);
  }
}

template <bool GIVEN_H, bool PEER = false>
int dispatch(Launch L, int threads, int per) {
  if (L.units == 0) return DRCVAR_OK;
  const bool vec = (reinterpret_cast<uintptr_t>(L.samples) % 16 == 0) && (L.s_obs % 2 == 0) &&
                   (L.s_step % 2 == 0) && (L.s_samp % 2 == 0);
  if (L.n > DRCVAR_MAX_SAMPLES) {  // beyond the register plans: the streaming kernel
    if (PEER || threads != 0 || per != 0) return DRCVAR_ERR_UNSUPPORTED;
    if (L.n > DRCVAR_MAX_SAMPLES_STREAM) return DRCVAR_ERR_UNSUPPORTED;
    (void)hipGetLastError();
    launch_stream<GIVEN_H>(L, vec);
    return hipGetLastError() == hipSuccess ? DRCVAR_OK : DRCVAR_ERR_LAUNCH;
  }
  const int p = pick_plan(L.n, threads, per);
  if (p < 0) return DRCVAR_ERR_UNSUPPORTED;
  (void)hipGetLastError();  // clear stale errors from unrelated work
  L.lone = lone_form(kPlans[p].per, PEER, L.units, device_cu_count());
  int rc = DRCVAR_OK;
  switch (p) {
    case 0: rc = launch_plan<64, 2, 7, GIVEN_H, PEER>(L, vec); break;
    case 1: rc = launch_plan<128, 4, 8, GIVEN_H, PEER>(L, vec); break;
    case 2: rc = launch_plan<256, 4, 9, GIVEN_H, PEER>(L, vec); break;
    case 3: rc = launch_plan<256, 8, 10, GIVEN_H, PEER>(L, vec); break;
    case 4: rc = launch_plan<256, 16, 10, GIVEN_H, PEER>(L, vec); break;
    case 5: rc = launch_plan<256, 20, 10, GIVEN_H, PEER>(L, vec); break;
    case 6: rc = launch_plan<512, 16, 10, GIVEN_H, PEER>(L, vec); break;
    case 7: rc = launch_plan<512, 20, 10, GIVEN_H, PEER>(L, vec); break;
    case 8: rc = launch_plan<1024, 12, 10, GIVEN_H, PEER>(L, vec); break;
    case 9: rc = launch_plan<1024, 16, 10, GIVEN_H, PEER>(L, vec); break;
    default:
      if constexpr (PEER) {
        return DRCVAR_ERR_UNSUPPORTED;  // tuning geometries: not in the peer form
      } else {
        switch (p) {
          case 10: rc = launch_plan<64, 16, 9, GIVEN_H, false>(L, vec); break;
          case 11: rc = launch_plan<128, 8, 9, GIVEN_H, false>(L, vec); break;
          case 12: rc = launch_plan<512, 2, 9, GIVEN_H, false>(L, vec); break;
          default: rc = launch_plan<1024, 10, 10, GIVEN_H, false>(L, vec); break;
        }
      }
  }
  if (rc != DRCVAR_OK) return rc;
  return hipGetLastError() == hipSuccess ? DRCVAR_OK : DRCVAR_ERR_LAUNCH;
}

int safe_halfspaces(const double* samples, int64_t n_obstacles, int64_t n_steps,
                    int64_t n_samples, int64_t stride_obstacle, int64_t stride_step,
                    int64_t stride_sample, const double* ego_ref_pos, int64_t ego_stride_step,
                    double robot_radius, double obstacle_radius, double alpha, double delta,
                    double epsilon, double* out, int32_t* status, void* stream, int threads,
                    int per, const drcvar_peer_set* peers = nullptr, int64_t row_base = 0) {
  if (n_obstacles < 0 || n_steps < 0 || n_samples < 1) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (!params_ok(robot_radius, obstacle_radius, alpha, delta, epsilon))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  const int64_t units = n_obstacles * n_steps;
  if (units == 0) return DRCVAR_OK;
  if (!samples || !ego_ref_pos || (!out && !peers) || units > 0x7fffffff)
    return DRCVAR_ERR_INVALID_ARGUMENT;
  Launch L{samples, units, n_steps, n_samples, stride_obstacle, stride_step, stride_sample,
           ego_ref_pos, 0, ego_stride_step,
           make_params(robot_radius, obstacle_radius, alpha, delta, epsilon, n_samples), out,
           status, static_cast<hipStream_t>(stream)};
  if (peers) {
    const drcvar_peer_set& ps = *peers;
    if (ps.n_ranks < 1 || ps.n_ranks > DRCVAR_MAX_PEERS || ps.rank < 0 || ps.rank >= ps.n_ranks ||
        !ps.state || ps.rows < 0 || row_base < 0 || row_base + units > ps.rows)
      return DRCVAR_ERR_INVALID_ARGUMENT;
    for (int j = 0; j < ps.n_ranks; ++j)
      if (!ps.region[j]) return DRCVAR_ERR_INVALID_ARGUMENT;
    for (int j = 0; j < DRCVAR_MAX_PEERS; ++j) L.peer.region[j] = j < ps.n_ranks ? ps.region[j] : nullptr;
    L.peer.rows = ps.rows;
    L.peer.row_base = row_base;
    L.peer.gen = ps.state;
    L.peer.n_ranks = ps.n_ranks;
    return dispatch<false, true>(L, 0, 0);
  }
  return dispatch<false>(L, threads, per);
}

}  // namespace

extern "C" {

#ifdef DRCVAR_STAMPS
// diagnostic build only (not part of the ABI header): copy the phase stamps to the host
int drcvar_diag_stamps(unsigned long long* host, int n_units) {
  const int n = n_units < kStampUnits ? n_units : kStampUnits;
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * n * kStamps,
                             0, hipMemcpyDeviceToHost) == hipSuccess ? n : -1;
}
#endif

int drcvar_abi_version(void) { return DRCVAR_ABI_VERSION; }

const char* drcvar_strerror(int code) {
  switch (code) {
    case DRCVAR_OK: return "ok";
    case DRCVAR_ERR_INVALID_ARGUMENT: return "invalid argument";
    case DRCVAR_ERR_UNSUPPORTED: return "n_samples beyond DRCVAR_MAX_SAMPLES_STREAM or no such launch geometry";
    case DRCVAR_ERR_LAUNCH: return "HIP kernel launch failed";
    default: return "unknown error";
  }
}

int drcvar_launch_plan(int64_t n_samples, int32_t* threads_per_unit, int32_t* samples_per_thread,
                       int32_t* bins) {
  if (n_samples < 1) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (n_samples > DRCVAR_MAX_SAMPLES) {  // streaming kernel: nothing per thread held on chip
    if (n_samples > DRCVAR_MAX_SAMPLES_STREAM) return DRCVAR_ERR_UNSUPPORTED;
    if (threads_per_unit) *threads_per_unit = kStreamBlock;
    if (samples_per_thread) *samples_per_thread = 0;
    if (bins) *bins = 1 << kStreamLogNB;
    return DRCVAR_OK;
  }
  const int p = pick_plan(n_samples, 0, 0);
  if (p < 0) return DRCVAR_ERR_UNSUPPORTED;
  if (threads_per_unit) *threads_per_unit = kPlans[p].block;
  if (samples_per_thread) *samples_per_thread = kPlans[p].per;
  if (bins) *bins = 1 << kPlans[p].log_nb;
  return DRCVAR_OK;
}

int drcvar_safe_halfspaces_f64(const double* samples, int64_t n_obstacles, int64_t n_steps,
                               int64_t n_samples, int64_t stride_obstacle, int64_t stride_step,
                               int64_t stride_sample, const double* ego_ref_pos,
                               int64_t ego_stride_step, double robot_radius,
                               double obstacle_radius, double alpha, double delta, double epsilon,
                               double* out, void* stream) {
  return safe_halfspaces(samples, n_obstacles, n_steps, n_samples, stride_obstacle, stride_step,
                         stride_sample, ego_ref_pos, ego_stride_step, robot_radius,
                         obstacle_radius, alpha, delta, epsilon, out, nullptr, stream, 0, 0);
}

int drcvar_safe_halfspaces_f64_ex(const double* samples, int64_t n_obstacles, int64_t n_steps,
                                  int64_t n_samples, int64_t stride_obstacle, int64_t stride_step,
                                  int64_t stride_sample, const double* ego_ref_pos,
                                  int64_t ego_stride_step, double robot_radius,
                                  double obstacle_radius, double alpha, double delta,
                                  double epsilon, double* out, void* stream,
                                  int32_t threads_per_unit, int32_t samples_per_thread) {
  if ((threads_per_unit == 0) != (samples_per_thread == 0)) return DRCVAR_ERR_INVALID_ARGUMENT;
  return safe_halfspaces(samples, n_obstacles, n_steps, n_samples, stride_obstacle, stride_step,
                         stride_sample, ego_ref_pos, ego_stride_step, robot_radius,
                         obstacle_radius, alpha, delta, epsilon, out, nullptr, stream,
                         threads_per_unit, samples_per_thread);
}

int drcvar_safe_halfspaces_f64_v2(const double* samples, int64_t n_obstacles, int64_t n_steps,
                                  int64_t n_samples, int64_t stride_obstacle, int64_t stride_step,
                                  int64_t stride_sample, const double* ego_ref_pos,
                                  int64_t ego_stride_step, double robot_radius,
                                  double obstacle_radius, double alpha, double delta,
                                  double epsilon, double* out, int32_t* status, void* stream,
                                  int32_t threads_per_unit, int32_t samples_per_thread) {
  if ((threads_per_unit == 0) != (samples_per_thread == 0)) return DRCVAR_ERR_INVALID_ARGUMENT;
  return safe_halfspaces(samples, n_obstacles, n_steps, n_samples, stride_obstacle, stride_step,
                         stride_sample, ego_ref_pos, ego_stride_step, robot_radius,
                         obstacle_radius, alpha, delta, epsilon, out, status, stream,
                         threads_per_unit, samples_per_thread);
}

int drcvar_safe_halfspaces_f64_peer(const double* samples, int64_t n_obstacles, int64_t n_steps,
                                    int64_t n_samples, int64_t stride_obstacle, int64_t stride_step,
                                    int64_t stride_sample, const double* ego_ref_pos,
                                    int64_t ego_stride_step, double robot_radius,
                                    double obstacle_radius, double alpha, double delta,
                                    double epsilon, const drcvar_peer_set* peers, int64_t row_base,
                                    int32_t* status, void* stream) {
  if (!peers) return DRCVAR_ERR_INVALID_ARGUMENT;
  return safe_halfspaces(samples, n_obstacles, n_steps, n_samples, stride_obstacle, stride_step,
                         stride_sample, ego_ref_pos, ego_stride_step, robot_radius,
                         obstacle_radius, alpha, delta, epsilon, nullptr, status, stream, 0, 0,
                         peers, row_base);
}

int drcvar_offsets_given_h_f64_v2(const double* samples, int64_t n_units, int64_t n_samples,
                                  int64_t stride_unit, int64_t stride_sample, const double* h,
                                  int64_t h_stride_unit, double robot_radius,
                                  double obstacle_radius, double alpha, double delta,
                                  double epsilon, double* out, int32_t* status, void* stream) {
  if (n_units < 0 || n_samples < 1) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (!params_ok(robot_radius, obstacle_radius, alpha, delta, epsilon))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  if (n_units == 0) return DRCVAR_OK;
  if (!samples || !h || !out || n_units > 0x7fffffff) return DRCVAR_ERR_INVALID_ARGUMENT;
  // units along the grid's x dimension: one "obstacle" of n_units steps
  Launch L{samples, n_units, n_units, n_samples, 0, stride_unit, stride_sample,
           h, 0, h_stride_unit,
           make_params(robot_radius, obstacle_radius, alpha, delta, epsilon, n_samples), out,
           status, static_cast<hipStream_t>(stream)};
  return dispatch<true>(L, 0, 0);
}

int drcvar_offsets_given_h_f64(const double* samples, int64_t n_units, int64_t n_samples,
                               int64_t stride_unit, int64_t stride_sample, const double* h,
                               int64_t h_stride_unit, double robot_radius, double obstacle_radius,
                               double alpha, double delta, double epsilon, double* out,
                               void* stream) {
  return drcvar_offsets_given_h_f64_v2(samples, n_units, n_samples, stride_unit, stride_sample, h,
                                       h_stride_unit, robot_radius, obstacle_radius, alpha, delta,
                                       epsilon, out, nullptr, stream);
}

}  // extern "C"
#endif  // !DRCVAR_HOST_PLANS_ONLY
