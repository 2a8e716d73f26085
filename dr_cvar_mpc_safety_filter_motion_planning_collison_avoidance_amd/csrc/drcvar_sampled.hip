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
// The wave reductions, the bucket map, the histogram scan and the candidate ranking are copies of
// the helpers in drcvar_halfspace.hip: that file is left byte-identical because the committed
// counter pass (profiles/kernel_time.json) is keyed to its hash.  Sharing them through an .inc is
// a later change, together with a re-run of that pass.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "drcvar_sampling.h"

namespace {

constexpr int kWave = 64;
constexpr int kCap = 128;          // candidates ranked directly (per-wave region size in LDS)
constexpr int kMaxValueIters = 3;  // value-linear refinements before switching to integer keys
constexpr double kSentinel = 100.0;

#include "drcvar_generator.inc"

// Launch-uniform scalars of the halfspace mathematics (make_params, as the stored form makes them).
struct Params {
  double rc, alpha, delta, epsilon, eps_over_alpha;
  double inv_n, k, inv_k;
  double z_alpha, window_sd, z_lo, hist_scale;
  uint32_t rank;
  int unbounded;
  double degenerate_sq;
};

// The draw's launch-uniform arguments (the sampler's SampleArgs, without its output).
struct DrawArgs {
  int64_t T, nom_so, nom_st, ego_st, u0, su, sn;
  int n;
  int zero_first;
  double l00, l10, l11;
  PhiloxUniform pu;
  LogScale lg;
};

// The pair of samples of one Philox call: the sampler's draw_pair, restated (drcvar_sampling.hip).
template <bool kIso>
__device__ __forceinline__ void draw_pair(uint64_t g, const DrawArgs& a, double nx, double ny,
                                          const double* s_turn, const double* s_log, double* x0,
                                          double* y0, double* x1, double* y1) {
  const Philox r = philox4x32_10(static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32), a.pu);
  double c0, sn0, c1, sn1;
  const double rad0 = sqrt_normal(scaled_neg2_log_u32(r.x[0], s_log, a.lg));
  cos_sin_u32(r.x[1], s_turn, &c0, &sn0);
  const double rad1 = sqrt_normal(scaled_neg2_log_u32(r.x[2], s_log, a.lg));
  cos_sin_u32(r.x[3], s_turn, &c1, &sn1);
  if constexpr (kIso) {
    *x0 = fma(rad0, c0, nx);
    *y0 = fma(rad0, sn0, ny);
    *x1 = fma(rad1, c1, nx);
    *y1 = fma(rad1, sn1, ny);
  } else {
    const double z00 = rad0 * c0, z01 = rad0 * sn0, z10 = rad1 * c1, z11 = rad1 * sn1;
    *x0 = fma(a.l00, z00, nx);
    *y0 = fma(a.l10, z00, fma(a.l11, z01, ny));
    *x1 = fma(a.l00, z10, nx);
    *y1 = fma(a.l10, z10, fma(a.l11, z11, ny));
  }
}

// ---------------------------------------------------------------------------------------------
// copies of drcvar_halfspace.hip's device helpers (see the note at the top)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double rsqrt_nr(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  return y * fma(-0.5 * x * y, y, 1.5);
}

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
constexpr int kDppQuadXor1 = 0xB1;     // quad_perm [1,0,3,2]
constexpr int kDppQuadXor2 = 0x4E;     // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141;  // row_half_mirror
constexpr int kDppMirror = 0x140;      // row_mirror

struct OpAdd {
  __device__ static double f(double a, double b) { return a + b; }
};
struct OpMin {
  __device__ static double f(double a, double b) { return fmin(a, b); }
};
struct OpMax {
  __device__ static double f(double a, double b) { return fmax(a, b); }
};

__device__ __forceinline__ double uniform_f64(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

template <class Op>
__device__ __forceinline__ double swap_combine16(double v) {
  const auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(v), __double2loint(v), false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(v), __double2hiint(v), false, false);
  return Op::f(__hiloint2double(hi[0], lo[0]), __hiloint2double(hi[1], lo[1]));
}
template <class Op>
__device__ __forceinline__ double swap_combine32(double v) {
  const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(v), __double2loint(v), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(v), __double2hiint(v), false, false);
  return Op::f(__hiloint2double(hi[0], lo[0]), __hiloint2double(hi[1], lo[1]));
}

// Uniform across the wave, bitwise: every lane evaluates the same tree.  All 64 lanes active.
template <class Op>
__device__ __forceinline__ double wave_reduce(double v) {
  v = Op::f(v, dpp_f64<kDppQuadXor1>(v));
  v = Op::f(v, dpp_f64<kDppQuadXor2>(v));
  v = Op::f(v, dpp_f64<kDppHalfMirror>(v));
  v = Op::f(v, dpp_f64<kDppMirror>(v));
  return uniform_f64(swap_combine32<Op>(swap_combine16<Op>(v)));
}

// Sum of NW per-wave partials read by every thread (broadcast LDS reads), fixed pairwise tree.
template <int NW>
__device__ __forceinline__ double sum_partials(const double* p) {
  double v[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) v[w] = p[w];
#pragma unroll
  for (int stride = 1; stride < NW; stride *= 2)
#pragma unroll
    for (int w = 0; w + stride < NW; w += 2 * stride) v[w] = v[w] + v[w + stride];
  return uniform_f64(v[0]);
}

template <class Op>
__device__ __forceinline__ double identity_of();
template <>
__device__ __forceinline__ double identity_of<OpAdd>() { return 0.0; }
template <>
__device__ __forceinline__ double identity_of<OpMin>() { return INFINITY; }
template <>
__device__ __forceinline__ double identity_of<OpMax>() { return -INFINITY; }

// Workgroup reduction of one value; `slot` is LDS scratch of NW doubles owned by the call site.
template <class Op, int NW>
__device__ __forceinline__ double block_reduce(double v, double* slot) {
  v = wave_reduce<Op>(v);
  if constexpr (NW > 1) {
    const int lane = threadIdx.x & (kWave - 1);
    const int w = threadIdx.x / kWave;
    if (lane == 0) slot[w] = v;
    __syncthreads();
    v = wave_reduce<Op>(lane < NW ? slot[lane] : identity_of<Op>());
  }
  return v;
}

// order-preserving map double -> uint64 (total order on non-NaN values)
__device__ __forceinline__ uint64_t f64_key(double d) {
  const uint64_t u = static_cast<uint64_t>(__double_as_longlong(d));
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

// Monotone (non-decreasing) map of the candidate interval [lo, hi] onto NB histogram bins.
template <int LOG_NB>
struct BucketMap {
  static constexpr int NB = 1 << LOG_NB;
  bool value_mode;
  double lo, scale;
  uint64_t klo;
  int shift;

  __device__ __forceinline__ void init_range(double lo_, double hi_, int iter) {
    lo = lo_;
    const double range = hi_ - lo_;
    scale = static_cast<double>(NB) / range;
    value_mode = iter < kMaxValueIters && range > 0.0 && scale < 1e300 && range * scale >= 1.0;
    klo = f64_key(lo_);
    const uint64_t diff = f64_key(hi_) - klo;  // >= 1 when hi > lo
    const int bits = 64 - __builtin_clzll(diff | 1ull);
    shift = bits > LOG_NB ? bits - LOG_NB : 0;
  }
  __device__ __forceinline__ int operator()(double d) const {
    if (value_mode) {
      const double t = fmin(fmax((d - lo) * scale, 0.0), static_cast<double>(NB - 1));
      return static_cast<int>(t);
    }
    return static_cast<int>((f64_key(d) - klo) >> shift);  // key mode: lo <= d <= hi only
  }
};

struct ScanResult {
  int bin;
  uint32_t below, cnt;
  bool found;  // false when the histogram holds fewer than rr + 1 samples
};

// Histogram storage: lane l of a scanning wave owns bins [l B, (l + 1) B), B = NB / 64; one padding
// word after every B bins makes the owner reads conflict-free.
template <int NB>
__device__ __forceinline__ int hist_slot(int bin) {  // bin >= 0
  constexpr unsigned B = NB / kWave;
  const unsigned b = static_cast<unsigned>(bin);
  return static_cast<int>(b + b / B);
}
template <int NB>
constexpr int hist_words() {
  return NB + kWave;
}

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x, int lane) {
  constexpr int kRowShr1 = 0x111, kRowShr2 = 0x112, kRowShr4 = 0x114, kRowShr8 = 0x118;
  int v = static_cast<int>(x);
  v += __builtin_amdgcn_update_dpp(0, v, kRowShr1, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, kRowShr2, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, kRowShr4, 0xF, 0xF, true);
  v += __builtin_amdgcn_update_dpp(0, v, kRowShr8, 0xF, 0xF, true);
  const int r0 = __builtin_amdgcn_readlane(v, 15);
  const int r1 = __builtin_amdgcn_readlane(v, 31);
  const int r2 = __builtin_amdgcn_readlane(v, 47);
  const int row = lane >> 4;
  v += (row >= 1 ? r0 : 0) + (row >= 2 ? r1 : 0) + (row >= 3 ? r2 : 0);
  return static_cast<uint32_t>(v);
}

// Any wave: the bin holding the sample of rank rr (0-based) and the counts below / inside it.
// Result is uniform across the wave.
template <int NB>
__device__ __forceinline__ ScanResult scan_bins(const uint32_t* hist, uint32_t rr, int lane) {
  constexpr int B = NB / kWave;  // contiguous bins per lane
  uint32_t h[B];
  const uint32_t* mine = hist + lane * (B + 1);
#pragma unroll
  for (int q = 0; q < B; ++q) h[q] = mine[q];
  uint32_t s = 0;
#pragma unroll
  for (int q = 0; q < B; ++q) s += h[q];
  const uint32_t incl = wave_inclusive_scan(s, lane);
  const unsigned long long hit = __ballot(incl > rr);
  if (hit == 0ull) return ScanResult{0, 0u, 0u, false};
  const int owner = __ffsll(static_cast<long long>(hit)) - 1;  // uniform
  uint32_t cum = incl - s;
  int bin = lane * B + B - 1;
  uint32_t below = 0, cnt = 0;
  bool done = false;
#pragma unroll
  for (int q = 0; q < B; ++q) {
    const bool take = !done && cum + h[q] > rr;
    bin = take ? lane * B + q : bin;
    below = take ? cum : below;
    cnt = take ? h[q] : cnt;
    done = done || take;
    cum += h[q];
  }
  return ScanResult{__builtin_amdgcn_readlane(bin, owner),
                    static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(below), owner)),
                    static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cnt), owner)),
                    true};
}

__device__ __forceinline__ bool in_range(double d, double lo, double hi) {
  return lo <= d && d <= hi;  // false for NaN
}

// MeanSafeHalfspace (core/halfspaces.py:84-94): direction from the ORIGIN, offset
// -(h.mu - R_c |h|), with compute_separating_vector's [1, 0] fallback
__device__ __forceinline__ void mean_halfspace(double mux, double muy, double rc, double* m0,
                                               double* m1, double* g) {
  const double nm = sqrt(mux * mux + muy * muy);
  const bool degenerate = nm < 1e-10;
  *m0 = degenerate ? 1.0 : mux / nm;
  *m1 = degenerate ? 0.0 : muy / nm;
  *g = -((*m0 * mux + *m1 * muy) - rc * sqrt(*m0 * *m0 + *m1 * *m1));
}

// d_i = h . xi_i (core/risk_metrics.py:145,233: h @ samples.T)
__device__ __forceinline__ double project(double h0, double h1, double x, double y) {
  return fma(h0, x, h1 * y);
}

// Value-linear position in the window: t(d) = d scale + off (one fma, rounded once, so monotone
// non-decreasing in d for any scale > 0).  Below the window t < 0, inside 0 <= t < NB, above (and
// the +inf padding) t >= NB.
struct LinearMap {
  double scale, off;
  __device__ __forceinline__ double operator()(double d) const { return fma(d, scale, off); }
};

// Per-wave ordered compaction step: append the candidates of one row to this wave's LDS region.
__device__ __forceinline__ void append_candidate(double* region, uint32_t& wbase, bool is_cand,
                                                 double v, unsigned long long lt_mask) {
  const unsigned long long ballot = __ballot(is_cand);
  if (is_cand) region[wbase + __popcll(ballot & lt_mask)] = v;
  wbase += static_cast<uint32_t>(__popcll(ballot));
}

// Wave 0 (all lanes active): tau = the candidate of rank rr among the c <= kCap candidates held in
// per-wave regions cand[w kCap + i], i < wcount[w] (global order: wave, then position — fixed), and
// s_cand = sum over candidates below tau of (cand - tau), in candidate order.
template <int NW, int Q>
__device__ __forceinline__ double rank_candidates_q(const double* cand, uint32_t cw, uint32_t c,
                                                    uint32_t rr, int lane, double* s_cand) {
  int slot[2] = {-1, -1};
  uint32_t acc = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const uint32_t nw = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cw), w));
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const uint32_t g = lane + q * kWave;
      if (g >= acc && g < acc + nw) slot[q] = w * kCap + static_cast<int>(g - acc);
    }
    acc += nw;
  }
  double mine[2] = {NAN, NAN};  // candidates g = lane, lane + 64
#pragma unroll
  for (int q = 0; q < Q; ++q)
    if (slot[q] >= 0) mine[q] = cand[slot[q]];
  uint32_t less[2] = {0u, 0u}, eq[2] = {0u, 0u};
  double sl[2] = {0.0, 0.0};
  const uint32_t c0 = c < kWave ? c : kWave;
  for (uint32_t i = 0; i < c0; ++i) {  // uniform trip count
    const double z = readlane_f64(mine[0], static_cast<int>(i));
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const bool lt = z < mine[q];
      less[q] += lt ? 1u : 0u;
      eq[q] += (z == mine[q]) ? 1u : 0u;
      sl[q] += lt ? z - mine[q] : 0.0;
    }
  }
  for (uint32_t i = kWave; Q == 2 && i < c; ++i) {
    const double z = readlane_f64(mine[1], static_cast<int>(i - kWave));
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const bool lt = z < mine[q];
      less[q] += lt ? 1u : 0u;
      eq[q] += (z == mine[q]) ? 1u : 0u;
      sl[q] += lt ? z - mine[q] : 0.0;
    }
  }
  bool found = false;
  double found_v = 0.0, found_s = 0.0;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    if (lane + q * kWave < c && less[q] <= rr && rr < less[q] + eq[q]) {
      found = true;
      found_v = mine[q];
      found_s = sl[q];
    }
  }
  const unsigned long long fb = __ballot(found);
  const int src = __ffsll(static_cast<long long>(fb)) - 1;
  *s_cand = readlane_f64(found_s, src);
  return readlane_f64(found_v, src);
}
template <int NW>
__device__ __forceinline__ double rank_candidates(const double* cand, uint32_t cw, uint32_t c,
                                                  uint32_t rr, int lane, double* s_cand) {
  return c <= static_cast<uint32_t>(kWave) ? rank_candidates_q<NW, 1>(cand, cw, c, rr, lane, s_cand)
                                           : rank_candidates_q<NW, 2>(cand, cw, c, rr, lane, s_cand);
}

// 1/sqrt(x) within 1.5 units of 2^-53: rsqrt_nr leaves 2.5 roundings plus 1.5 e^2 of the hardware
// seed's error e (about 5 units in all, measured on a unit with |h1| = 0.8: h1 five units off, more
// than the four the reference's bound on h allots to the subtraction, the rsqrt and the product).
// One more Newton step in residual form: r = x y is rounded once, 1 - r y comes exact out of the
// fma, and y (1 + e / 2) rounds once.
__device__ __forceinline__ double rsqrt_nr2(double x) {
  const double y = rsqrt_nr(x);
  const double e = fma(-(x * y), y, 1.0);
  return fma(0.5 * e, y, y);
}

// compute_separating_vector(ego, mu) (core/geometry.py:35-53): (mu - ego) / |mu - ego|, [1, 0]
// below 1e-10 (rsqrt + Newton).
__device__ __forceinline__ void separating_direction(double mux, double muy, double e0, double e1,
                                                     double deg_sq, double* h0, double* h1) {
  const double dx = mux - e0, dy = muy - e1;
  const double n2 = dx * dx + dy * dy;
  const double inv = n2 == INFINITY ? 0.0 : rsqrt_nr2(n2);
  const bool degenerate = n2 < deg_sq;
  *h0 = degenerate ? 1.0 : dx * inv;
  *h1 = degenerate ? 0.0 : dy * inv;
}

// |h| for R_c |h| (risk_metrics.py:293, :234): sqrt(1 + e) = 1 + e/2 - e^2/8 near a unit vector.
__device__ __forceinline__ double norm_h(double h0, double h1) {
  const double n2 = h0 * h0 + h1 * h1;
  const double e = n2 - 1.0;
  if (fabs(e) < 0x1p-40) return 1.0 + fma(-0.125 * e, e, 0.5 * e);  // uniform branch
  return sqrt(n2);
}

// Per-unit status word (DRCVAR_UNIT_*), as the stored form reports it.
__device__ __forceinline__ int32_t failure_status(bool nonfinite, const Params& prm) {
  return (nonfinite ? DRCVAR_UNIT_NONFINITE : 0) | (prm.unbounded ? DRCVAR_UNIT_UNBOUNDED : 0) |
         (prm.epsilon < 0.0 ? DRCVAR_UNIT_DR_UNBOUNDED : 0);
}

// The whole record by one lane, plain stores.
__device__ __forceinline__ void store_record(double* rec, double mux, double muy, double rc,
                                             double h0, double h1, double gc, double gs,
                                             double gt) {
  double m0, m1, gm;
  mean_halfspace(mux, muy, rc, &m0, &m1, &gm);
  rec[DRCVAR_COL_MEAN_H0] = m0;
  rec[DRCVAR_COL_MEAN_H1] = m1;
  rec[DRCVAR_COL_G_MEAN] = gm;
  rec[DRCVAR_COL_H0] = h0;
  rec[DRCVAR_COL_H1] = h1;
  rec[DRCVAR_COL_G_CVAR] = gc;
  rec[DRCVAR_COL_G_DR_STAR] = gs;
  rec[DRCVAR_COL_G_DR_TILDE] = gt;
}

// Exact selection over the register-held projections d[0..Q) (bit q of vmask: slot q holds a
// sample), for the units the window does not finish.  The structure of the stored form's
// select_from_memory with its re-reads replaced by the registers: exact min/max, then histogram
// refinement (value-linear, then order-preserving integer keys) until <= kCap candidates remain or
// the run collapses to one value.  Result (valid in wave 0): tau and dsum = sum_{d<tau} (d - tau).
template <int BLOCK, int LOG_NB, int Q>
__device__ __forceinline__ void select_from_registers(const double (&d)[Q], uint32_t vmask,
                                                      double mu_d, uint32_t rank, uint32_t* hist,
                                                      double* cand, uint32_t* wcount,
                                                      double* red_rng, double* red_tail,
                                                      double* tau_out, double* dsum_out) {
  constexpr int NW = BLOCK / kWave;
  constexpr int NB = 1 << LOG_NB;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid / kWave;
  __syncthreads();  // the window path's readers of hist are done

  double vmin = INFINITY, vmax = -INFINITY;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    if ((vmask >> q) & 1u) {
      vmin = fmin(vmin, d[q]);
      vmax = fmax(vmax, d[q]);
    }
  }
  double lo = block_reduce<OpMin, NW>(vmin, red_rng);
  double hi = block_reduce<OpMax, NW>(vmax, red_rng + NW);
  if (lo == hi) {  // every sample projects to one value: no tail below it
    *tau_out = lo;
    *dsum_out = 0.0;
    return;  // uniform
  }
  uint32_t rr = rank, c = 0;
  bool have_bin = false, tau_known = false;
  double tau = lo;
  int bin = 0;
  BucketMap<LOG_NB> map;
  for (int iter = 0; !tau_known; ++iter) {
    map.init_range(lo, hi, iter);
    for (int b = tid; b < hist_words<NB>(); b += BLOCK) hist[b] = 0u;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const double v = ((vmask >> q) & 1u) ? d[q] : NAN;
      if (in_range(v, lo, hi)) atomicAdd(&hist[hist_slot<NB>(map(v))], 1u);
    }
    __syncthreads();
    const ScanResult sr = scan_bins<NB>(hist, rr, lane);
    bin = sr.bin;
    rr -= sr.below;
    c = sr.cnt;
    have_bin = true;
    if (c <= kCap) break;
    double rmin = INFINITY, rmax = -INFINITY;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const double v = ((vmask >> q) & 1u) ? d[q] : NAN;
      if (in_range(v, lo, hi) && map(v) == bin) {
        rmin = fmin(rmin, v);
        rmax = fmax(rmax, v);
      }
    }
    __syncthreads();  // all waves have scanned hist before it is cleared again
    lo = block_reduce<OpMin, NW>(rmin, red_rng);
    hi = block_reduce<OpMax, NW>(rmax, red_rng + NW);
    have_bin = false;
    if (lo == hi) {
      tau_known = true;
      tau = lo;
    }
  }

  double sq = 0.0;
  uint32_t wbase = 0;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
#pragma unroll
  for (int q = 0; q < Q; ++q) {  // uniform trip count: ballots see whole waves
    const double v = ((vmask >> q) & 1u) ? d[q] : NAN;
    const bool inr = in_range(v, lo, hi);
    const int bj = (have_bin && inr) ? map(v) : 0;
    const bool below = v < lo || (have_bin && inr && bj < bin);
    if (below) sq += v - mu_d;
    append_candidate(cand + wave * kCap, wbase, !tau_known && inr && (!have_bin || bj == bin), v,
                     lt_mask);
  }
  sq = wave_reduce<OpAdd>(sq);
  if (lane == 0) {
    red_tail[wave] = sq;
    wcount[wave] = wbase;
  }
  __syncthreads();
  if (wave != 0) return;
  const double s_below = sum_partials<NW>(red_tail);
  double s_cand = 0.0;
  if (!tau_known)
    tau = rank_candidates<NW>(cand, lane < NW ? wcount[lane] : 0u, c, rr, lane, &s_cand);
  const double n_below = static_cast<double>(rank - rr);
  *tau_out = tau;
  *dsum_out = (s_below - n_below * (tau - mu_d)) + s_cand;
}

// ---------------------------------------------------------------------------------------------
// the kernel
//   BLOCK    threads per unit (one workgroup per unit)
//   PP       Philox pairs per thread (N <= 2 BLOCK PP)
//   LOG_NB   log2 of the histogram bins
//   ISO      the sampler's isotropic LogScale form
// Blocks of 512 threads are held to 128 VGPRs (four waves per SIMD): two workgroups share a CU,
// so one unit's draw (VALU) overlaps the other's selection (barriers, LDS, one ranking wave).
// ---------------------------------------------------------------------------------------------
template <int BLOCK, int PP, int LOG_NB, bool ISO>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(BLOCK >= 512 ? 4 : 1)))
sampled_halfspace_kernel(const double* __restrict__ nominal, const double* __restrict__ ego,
                         DrawArgs a, Params prm, double* __restrict__ out,
                         int32_t* __restrict__ status, double* __restrict__ samples_out) {
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
  const double* nom = nominal + o * a.nom_so + t * a.nom_st;
  const double nx = nom[0], ny = nom[1];
  const double* ep = ego + t * a.ego_st;
  const double e0 = ep[0], e1 = ep[1];
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
  const uint64_t g0 = static_cast<uint64_t>(u) * static_cast<uint64_t>(pairs) + static_cast<uint64_t>(tid);
#pragma unroll
  for (int j = 0; j < PP; ++j) {
    const int p = tid + j * BLOCK;
    if (p < pairs) vmask |= 1u << (2 * j);
    if (p + pairs < n) vmask |= 2u << (2 * j);
    x[2 * j] = x[2 * j + 1] = nx;
    y[2 * j] = y[2 * j + 1] = ny;
    // a whole wave past the unit's pairs skips the call; idle lanes of a partly filled wave make
    // it on a counter of their own and drop the result
    if (noisy && wave_first + j * BLOCK < pairs)
      draw_pair<ISO>(g0 + static_cast<uint64_t>(j * BLOCK), a, nx, ny, s_turn, s_log, &x[2 * j],
                     &y[2 * j], &x[2 * j + 1], &y[2 * j + 1]);
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
  separating_direction(mux, muy, e0, e1, prm.degenerate_sq, &h0, &h1);
  if (bad || prm.unbounded) {  // risk_metrics.py:298-303,334-338
    if (tid == 0) {
      const double r = prm.rc * norm_h(h0, h1);
      store_record(rec, mux, muy, prm.rc, h0, h1, kSentinel, kSentinel, kSentinel - r);
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
      select_from_registers<BLOCK, LOG_NB, Q>(d, vmask, mu_d, rank, hist, cand, wcount, red_rng,
                                              red_tail, &tau, &dsum);
    } else {  // every sample is the nominal point: tau = its projection, no tail below it
      tau = project(h0, h1, nx, ny);
      dsum = 0.0;
    }
    if (wave != 0) return;
  }

  // ---- 5. offsets (wave 0, lane 0) -------------------------------------------------------------
  if (lane == 0) {
    const double r = prm.rc * norm_h(h0, h1);  // R_c |h| (risk_metrics.py:293, :234)
    const double L = tau + dsum * prm.inv_k;   // lower-tail mean
    const double g_cvar = r - prm.delta - L;
    double g_star = kSentinel, g_tilde = kSentinel - r;
    if (prm.epsilon >= 0.0) {  // else: DR LP unbounded (lambda -> inf), solver-failure sentinel
      g_star = r - prm.delta + prm.eps_over_alpha - L;
      g_tilde = g_star - r;
    }
    store_record(rec, mux, muy, prm.rc, h0, h1, g_cvar, g_star, g_tilde);
    if (status) status[row] = failure_status(false, prm);
  }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// LogScale for lam (see drcvar_generator.inc), as the sampler makes it.
LogScale make_log_scale(double lam) {
  LogScale c{};
  c.lam = lam;
  c.q0 = lam * (1.0 / 192.0);
  c.q1 = lam * (1.0 / 80.0);
  c.q2 = lam * (1.0 / 32.0);
  c.q3 = lam * (1.0 / 12.0);
  c.q4 = lam * 0.25;
  const long double e2 = -2.0L * static_cast<long double>(lam) * 0.693147180559945309417232121458176568L;
  double eh = static_cast<double>(e2);
  uint64_t bits;
  std::memcpy(&bits, &eh, sizeof bits);
  bits &= ~uint64_t{0x7f};  // 53 - 7 = 46 significant bits
  std::memcpy(&eh, &bits, sizeof bits);
  c.eh = eh;
  c.el = static_cast<double>(e2 - static_cast<long double>(eh));
  return c;
}

// Standard-normal quantile (P. J. Acklam's rational approximation) — only positions the window.
double normal_quantile(double p) {
  static const double a[] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02,
                             1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00};
  static const double b[] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02,
                             6.680131188771972e+01, -1.328068155288572e+01};
  static const double c[] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00,
                             -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00};
  static const double d[] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00,
                             3.754408661907416e+00};
  p = std::fmin(std::fmax(p, 1e-12), 1.0 - 1e-12);
  const double plow = 0.02425;
  if (p < plow) {
    const double q = std::sqrt(-2.0 * std::log(p));
    return (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) /
           ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.0);
  }
  if (p > 1.0 - plow) return -normal_quantile(1.0 - p);
  const double q = p - 0.5, r = q * q;
  return (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q /
         (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0);
}

// The stored form's make_params (drcvar_halfspace.hip): the same z_lo, window_sd and rank.
Params make_params(double rr, double ro, double alpha, double delta, double eps, int64_t n) {
  Params p{};
  p.rc = rr + ro;
  p.alpha = alpha;
  p.delta = delta;
  p.epsilon = eps;
  p.eps_over_alpha = eps / alpha;
  const double dn = static_cast<double>(n);
  p.inv_n = 1.0 / dn;
  p.k = alpha * dn;  // exactly as the reference forms alpha * n_samples
  p.inv_k = 1.0 / p.k;
  p.unbounded = !(p.k <= dn);
  const int64_t m = static_cast<int64_t>(std::floor(p.k));
  p.rank = static_cast<uint32_t>(p.unbounded ? 0 : (m < n - 1 ? m : n - 1));
  // window: the Gaussian alpha-quantile +- max(0.25 sd, 12 standard errors of the sample quantile)
  const double a = std::fmin(std::fmax(alpha, 1e-12), 1.0 - 1e-12);
  p.z_alpha = normal_quantile(a);
  const double phi = std::exp(-0.5 * p.z_alpha * p.z_alpha) * 0.3989422804014327;
  const double se = std::sqrt(a * (1.0 - a) / dn) / phi;
  p.window_sd = std::fmax(0.25, 12.0 * se);
  p.z_lo = p.z_alpha - p.window_sd;
  double t = 1e-20;  // smallest t with sqrt(t) >= 1e-10 (sqrt is correctly rounded and monotone)
  while (std::sqrt(t) >= 1e-10) t = std::nextafter(t, 0.0);
  while (std::sqrt(t) < 1e-10) t = std::nextafter(t, 1.0);
  p.degenerate_sq = t;
  return p;
}

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
  int64_t count;
  bool iso;
  hipStream_t stream;
};

template <int BLOCK, int PP, int LOG_NB>
void launch_plan(Launch L) {
  L.prm.hist_scale = static_cast<double>(1 << LOG_NB) / (2.0 * L.prm.window_sd);
  const dim3 grid(static_cast<unsigned>(L.count)), block(BLOCK);
  if (L.iso)
    hipLaunchKernelGGL((sampled_halfspace_kernel<BLOCK, PP, LOG_NB, true>), grid, block, 0, L.stream,
                       L.nominal, L.ego, L.a, L.prm, L.out, L.status, L.samples_out);
  else
    hipLaunchKernelGGL((sampled_halfspace_kernel<BLOCK, PP, LOG_NB, false>), grid, block, 0, L.stream,
                       L.nominal, L.ego, L.a, L.prm, L.out, L.status, L.samples_out);
}

}  // namespace

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
  if (n_obstacles < 0 || n_steps < 0 || n_samples < 0 || unit_begin < 0 || unit_count < 0)
    return DRCVAR_ERR_INVALID_ARGUMENT;
  if (!(l00 == l00) || !(l10 == l10) || !(l11 == l11)) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (!(std::isfinite(robot_radius) && std::isfinite(obstacle_radius) && std::isfinite(alpha) &&
        alpha > 0.0 && std::isfinite(delta) && std::isfinite(epsilon)))
    return DRCVAR_ERR_INVALID_ARGUMENT;
  // the sampler's grid limits, and the register plans' sample count
  if (n_obstacles > (int64_t{1} << 40) || n_steps > (int64_t{1} << 40) ||
      n_obstacles * n_steps > (int64_t{1} << 40) || n_samples > DRCVAR_MAX_SAMPLES)
    return DRCVAR_ERR_UNSUPPORTED;
  const int64_t units = n_obstacles * n_steps;
  if (unit_begin > units || unit_count > units - unit_begin) return DRCVAR_ERR_INVALID_ARGUMENT;
  if (unit_count == 0 || n_samples == 0) return DRCVAR_OK;
  if (!nominal || !ego || !out) return DRCVAR_ERR_INVALID_ARGUMENT;
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
  L.a.pu = make_philox_uniform(static_cast<uint32_t>(stream_offset),
                               static_cast<uint32_t>(stream_offset >> 32),
                               static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
  // the sampler's test for its isotropic form (launch_samples): the draws are the same bits only
  // if this kernel takes that form exactly when the sampler does
  const double lam = l00 * l00;
  L.iso = l10 == 0.0 && l00 == l11 && l00 > 0.0 && std::isfinite(l00) && lam >= 0x1.0p-200 &&
          lam <= 0x1.0p200;
  L.a.lg = make_log_scale(L.iso ? lam : 1.0);
  L.prm = make_params(robot_radius, obstacle_radius, alpha, delta, epsilon, n_samples);
  L.out = out;
  L.status = status;
  L.samples_out = samples_out;
  L.count = unit_count;
  L.stream = static_cast<hipStream_t>(stream);
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
