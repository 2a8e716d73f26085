// drcvar_selection.inc — the selection toolkit of the halfspace kernels: the launch-uniform Params
// and their host side (normal_quantile, make_params, params_ok), the wave and workgroup reductions,
// the bucket map, the histogram scan and the candidate ranking that give the exact order statistic,
// the exact fallback built from them (select_exact, over a memory or a register source of the
// unit's projections), and the small per-unit formulas (direction, mean halfspace, |h|, the offsets
// and the solver-failure offsets, status word).  Included inside
// the anonymous namespace of drcvar_halfspace.hip (samples read from memory) and
// drcvar_sampled.hip (samples drawn in the kernel), after <hip/hip_runtime.h>, <cmath>, <cstdint>
// and drcvar_halfspace.h.  It includes nothing itself — in particular not drcvar_generator.inc:
// the stored form's source key (_native.source_key) stays independent of sampler edits.

constexpr int kWave = 64;
constexpr int kCap = 128;          // candidates ranked directly (per-wave region size in LDS)
constexpr int kMaxValueIters = 3;  // value-linear refinements before switching to integer keys
constexpr double kSentinel = 100.0;  // the reference's offset for a failed solve

// Launch-uniform scalars, precomputed on the host so the per-unit critical path carries as few
// fp64 divisions as possible.
struct Params {
  double rc;              // robot_radius + obstacle_radius
  double alpha;
  double delta;
  double epsilon;
  double eps_over_alpha;  // lambda* epsilon (risk_metrics.py:110,122)
  double inv_n;           // 1 / N
  double inv_n0;          // 1 / size of the window's subsample (pilot: min(N, 64); row 0: min(N, threads))
  double k;               // alpha N
  double inv_k;           // 1 / (alpha N)
  double z_alpha;         // standard-normal alpha-quantile: centre of the fast-path window
  double window_sd;       // half-width of the fast-path window, in sd of d
  double z_lo;            // z_alpha - window_sd: low edge of the window, in sd of d
  double hist_scale;      // bins / (2 window_sd): bins per sd of d (set per launch plan)
  uint32_t rank;          // min(floor(alpha N), N - 1): 0-based rank of tau
  int unbounded;          // alpha N > N: both LPs unbounded (tau -> -inf), solver-failure sentinel
  double degenerate_sq;   // smallest x with sqrt(x) >= 1e-10: |v| < 1e-10  <=>  v.v < degenerate_sq
};

// 1/sqrt(x) to ~1 ulp: hardware seed + one Newton step (the exact sqrt + divide sequence is far
// longer and sits on the critical path of every unit)
__device__ __forceinline__ double rsqrt_nr(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  return y * fma(-0.5 * x * y, y, 1.5);
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

// ---------------------------------------------------------------------------------------------
// wave primitives: DPP row permutations (each an involution, so every lane of a row ends with the
// bitwise-identical value), then the four row results combined through readlane in fixed order
// ---------------------------------------------------------------------------------------------
// (mov_dpp, not update_dpp with an old value of 0: every lane of these permutations has a source,
// so the old value is never used, and materialising it cost two v_mov plus a DPP hazard wait per
// stage of every reduction on the chain)
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
constexpr int kDppQuadXor1 = 0xB1;    // quad_perm [1,0,3,2]
constexpr int kDppQuadXor2 = 0x4E;    // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141; // row_half_mirror
constexpr int kDppMirror = 0x140;     // row_mirror

struct OpAdd {
  __device__ static double f(double a, double b) { return a + b; }
};
struct OpMin {
  __device__ static double f(double a, double b) { return fmin(a, b); }
};
struct OpMax {
  __device__ static double f(double a, double b) { return fmax(a, b); }
};

// a wave-uniform value moved to SGPRs (keeps uniform scalars out of the VGPR budget)
__device__ __forceinline__ double uniform_f64(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float uniform_f32(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// gfx950 lane swaps: permlane16_swap exchanges odd rows of its first operand with even rows of
// its second, permlane32_swap the upper half of the first with the lower half of the second.
// With both operands = v, element [0] holds rows (0,0,2,2) / halves (lo,lo) and element [1] rows
// (1,1,3,3) / halves (hi,hi), so Op([0], [1]) combines row pairs / halves in every lane at once.
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

// Result is uniform across the wave (bitwise: every lane evaluates the same tree,
// ((r0 + r1) + (r2 + r3)) over the row results).  Requires all 64 lanes active.
// Measured (scripts/micro/reduce.hip): ~190 cycles latency, ~150 cycles per extra independent value.
template <class Op>
__device__ __forceinline__ double wave_reduce(double v) {
  v = Op::f(v, dpp_f64<kDppQuadXor1>(v));
  v = Op::f(v, dpp_f64<kDppQuadXor2>(v));
  v = Op::f(v, dpp_f64<kDppHalfMirror>(v));
  v = Op::f(v, dpp_f64<kDppMirror>(v));
  return uniform_f64(swap_combine32<Op>(swap_combine16<Op>(v)));
}

// Sum of NW per-wave partials p[0..NW) read by every thread (broadcast LDS reads), fixed
// pairwise tree — cheaper than a second wave reduction for the small NW of the launch plans.
// UNIFORM = false leaves the sum in VGPRs (every lane holds the same bits): for a caller whose next
// steps are vector arithmetic anyway and whose register budget has room.
template <int NW, class T, bool UNIFORM = true>
__device__ __forceinline__ T sum_partials(const T* p) {
  T v[NW];
#pragma unroll
  for (int w = 0; w < NW; ++w) v[w] = p[w];
#pragma unroll
  for (int stride = 1; stride < NW; stride *= 2)
#pragma unroll
    for (int w = 0; w + stride < NW; w += 2 * stride) v[w] = v[w] + v[w + stride];
  if constexpr (!UNIFORM) {
    return v[0];
  } else if constexpr (sizeof(T) == 8) {
    return uniform_f64(v[0]);
  } else {
    return uniform_f32(v[0]);
  }
}

template <class Op>
__device__ __forceinline__ double identity_of();
template <>
__device__ __forceinline__ double identity_of<OpAdd>() { return 0.0; }
template <>
__device__ __forceinline__ double identity_of<OpMin>() { return INFINITY; }
template <>
__device__ __forceinline__ double identity_of<OpMax>() { return -INFINITY; }

// Workgroup reduction of K values.  `slot` is LDS scratch of K*NW doubles owned by the call site
// (never reused by another call without a barrier in between).  The per-wave partials are
// combined by a second wave reduction (lane w holds wave w's partial), so the order is fixed.
template <class Op, int NW, int K>
__device__ __forceinline__ void block_reduce(double (&v)[K], double* slot) {
#pragma unroll
  for (int q = 0; q < K; ++q) v[q] = wave_reduce<Op>(v[q]);
  if constexpr (NW > 1) {
    const int lane = threadIdx.x & (kWave - 1);
    const int w = threadIdx.x / kWave;
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < K; ++q) slot[q * NW + w] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < K; ++q) {
      const double part = lane < NW ? slot[q * NW + lane] : identity_of<Op>();
      v[q] = wave_reduce<Op>(part);
    }
  }
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

  // exact range [lo_, hi_] of the candidates, lo_ < hi_: bucket(lo_) = 0 < bucket(hi_)
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

// Histogram storage: lane l of a scanning wave owns bins [l*B, (l+1)*B), B = NB/64.  One padding
// word after every B bins makes the owner reads conflict-free (lane stride B+1 words, B+1 odd).
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

// Inclusive prefix sum over the 64 lanes: DPP row shifts within each row of 16, then the row
// totals (lanes 15, 31, 47) added through readlane — no LDS round trips.
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

// This lane's bins of the histogram into registers — a step of its own so that a caller can issue
// the histogram reads together with its other post-barrier LDS reads.
template <int NB>
__device__ __forceinline__ void load_bins(const uint32_t* hist, int lane, uint32_t (&h)[NB / kWave]) {
  constexpr int B = NB / kWave;
  const uint32_t* mine = hist + lane * (B + 1);
#pragma unroll
  for (int q = 0; q < B; ++q) h[q] = mine[q];
}

// One level of the owner lane's bin search: pre[0 .. 2 W] are non-decreasing prefix counts with
// pre[0] <= rl < pre[2 W]; the half that holds the first prefix above rl is kept (a fresh array per
// level, all indices constants: selects between registers), k gains W when it is the upper one.
// At W = 1 the pair left is (lo, hi) = (pre[k], pre[k + 1]) of the first level's array.
template <int W>
__device__ __forceinline__ void halve_prefixes(const uint32_t (&pre)[2 * W + 1], uint32_t rl, int& k,
                                               uint32_t& lo, uint32_t& hi) {
  const bool up = pre[W] <= rl;
  k += up ? W : 0;
  if constexpr (W == 1) {
    lo = up ? pre[1] : pre[0];
    hi = up ? pre[2] : pre[1];
  } else {
    uint32_t half[W + 1];
#pragma unroll
    for (int i = 0; i <= W; ++i) half[i] = up ? pre[i + W] : pre[i];
    halve_prefixes<W / 2>(half, rl, k, lo, hi);
  }
}

// Any wave, its bins loaded (load_bins): the bin holding the sample of rank rr (0-based) and the
// counts below / inside it.  Result is uniform across the wave.
template <int NB>
__device__ __forceinline__ ScanResult scan_loaded_bins(const uint32_t (&h)[NB / kWave], uint32_t rr,
                                                      int lane) {
  constexpr int B = NB / kWave;  // contiguous bins per lane
  static_assert(B >= 2 && (B & (B - 1)) == 0, "the owner search halves a power-of-two run of bins");
  // pre[q] = samples of this lane's bins below bin q (pre[B] = the lane's total): independent of
  // the wave scan, so the adds fill its DPP wait states
  uint32_t pre[B + 1];
  pre[0] = 0u;
#pragma unroll
  for (int q = 0; q < B; ++q) pre[q + 1] = pre[q] + h[q];
  const uint32_t s = pre[B];
  const uint32_t incl = wave_inclusive_scan(s, lane);
  const unsigned long long hit = __ballot(incl > rr);
  if (hit == 0ull) return ScanResult{0, 0u, 0u, false};
  const int owner = __ffsll(static_cast<long long>(hit)) - 1;  // uniform
  // In the owner lane (the first with incl > rr) the samples below its bins number cum <= rr, and
  // the target is its bin k = #{q >= 1 : pre[q] <= rl}, rl = rr - cum < s: pre[] is non-decreasing,
  // so k comes from log2(B) compares, each keeping the half of pre[] that holds pre[k], pre[k + 1].
  // The other lanes compute values nobody reads (rl wraps there).
  const uint32_t cum = incl - s;
  const uint32_t rl = rr - cum;
  int k = 0;
  uint32_t lo, hi;  // pre[k], pre[k + 1]
  halve_prefixes<B / 2>(pre, rl, k, lo, hi);
  const int bin = lane * B + k;
  const uint32_t below = cum + lo, cnt = hi - lo;
  return ScanResult{__builtin_amdgcn_readlane(bin, owner),
                    static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(below), owner)),
                    static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cnt), owner)),
                    true};
}

template <int NB>
__device__ __forceinline__ ScanResult scan_bins(const uint32_t* hist, uint32_t rr, int lane) {
  uint32_t h[NB / kWave];
  load_bins<NB>(hist, lane, h);
  return scan_loaded_bins<NB>(h, rr, lane);
}

__device__ __forceinline__ bool in_range(double d, double lo, double hi) {
  return lo <= d && d <= hi;  // false for the NaN padding of idle slots
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

// d_i = h . xi_i — one expression, used both for register-resident samples and for re-reads, so
// both paths see bitwise-identical values (core/risk_metrics.py:145,233: h @ samples.T)
__device__ __forceinline__ double project(double h0, double h1, double x, double y) {
  return fma(h0, x, h1 * y);
}

// Value-linear position in the fast-path window: t(d) = d * scale + off (one fma, rounded once,
// so monotone non-decreasing in d for any scale > 0).  Below the window: t < 0; inside: 0 <= t <
// NB (bin = trunc(t) <= NB - 1); above it (and the +inf padding): t >= NB.
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

// The LDS byte address of a pointer into a __shared__ array (what a DS instruction takes).
__device__ __forceinline__ uint32_t lds_address(const void* p) {
  return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(
      (const __attribute__((address_space(3))) void*)p));
}

// append_candidate without its branch, for a workgroup that has its CU to itself (the kernel's
// LONE form): every lane computes its slot, and the one ds_write_b64 is issued under an exec mask
// narrowed to the ballot for that single instruction (saved, narrowed, restored inside one asm
// block), so the pass is straight-line code — the compiler keeps an s_cbranch_execz around any
// conditional block that holds a DS instruction.  On a full CU that skip is the cheaper form (a
// wave without a candidate issues nothing for the row); alone on a CU only the wave's own chain
// counts, and the branch is what costs.  Preconditions: all 64 lanes active on entry (BLOCK a
// multiple of 64, the call under uniform branches only); `region` points into LDS.  A zero ballot
// is legal: the store issues with an empty mask and writes nothing.  A lane outside the ballot
// never stores, so its slot (below wbase + 64) need not lie inside the region.
// The compiler does not count this store in lgkmcnt: a caller waits with lds_masked_wait() ahead
// of the barrier that publishes the region.
__device__ __forceinline__ void append_candidate_masked(double* region, uint32_t& wbase,
                                                        bool is_cand, double v,
                                                        unsigned long long lt_mask) {
  const unsigned long long ballot = __ballot(is_cand);
  const uint32_t addr = lds_address(region + wbase + __popcll(ballot & lt_mask));
  unsigned long long saved;
  asm volatile(
      "s_and_saveexec_b64 %0, %1\n\t"
      "ds_write_b64 %2, %3\n\t"
      "s_mov_b64 exec, %0"
      : "=&s"(saved)
      : "s"(ballot), "v"(addr), "v"(v)
      : "memory", "scc");
  wbase += static_cast<uint32_t>(__popcll(ballot));
}

// Every LDS operation of this wave has completed, the masked stores (which the compiler does not
// see) included: ahead of the barrier that publishes what they wrote.
__device__ __forceinline__ void lds_masked_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// One lane's tally of the express ranking against its own candidate `mine`: #{z < mine},
// #{z == mine} and sum_{z < mine} (z - mine) over the candidates z visited so far.
struct RankTally {
  uint32_t less = 0u, eq = 0u;
  double sl = 0.0;
};

// One visit of the express ranking: the candidate of the lowest lane left in the ballot `m` (taken
// in scalar code, m != 0) leaves the ballot and enters every lane's tally.
__device__ __forceinline__ void visit_candidate(double mine, unsigned long long& m, RankTally& t) {
  const int src = __builtin_ctzll(m);
  m &= m - 1ull;
  const double z = readlane_f64(mine, src);
  const bool lt = z < mine;
  t.less += lt ? 1u : 0u;
  t.eq += (z == mine) ? 1u : 0u;
  t.sl += lt ? z - mine : 0.0;
}

// The end of the express ranking: tau is the candidate of the first valid lane whose tally places
// rank rr on it, and that lane holds s_cand itself, so no reduction follows the ranking.
__device__ __forceinline__ double ranked_candidate(double mine, bool valid, const RankTally& t,
                                                   uint32_t rr, double* s_cand) {
  const bool found = valid && t.less <= rr && rr < t.less + t.eq;
  const unsigned long long fb = __ballot(found);
  const int src = __ffsll(static_cast<long long>(fb)) - 1;
  *s_cand = readlane_f64(t.sl, src);
  return readlane_f64(mine, src);
}

// Wave 0 (all lanes active), a target bucket of c <= 64 / NW candidates: no wave holds more than
// E = 64 / NW of them, so wave w appends its candidates to the segment cand[w * E + k] and all of
// the unit's candidates lie in cand[0 .. 64), in rank_candidates' order (wave, then position)
// with holes.  Lane l holds `mine` = cand[l] and `cnt` = wcount[l / E], and is a candidate iff
// l % E < cnt — the caller issues both reads in one batch with its other post-barrier reads, so
// nothing here computes a slot or waits on LDS again.  The candidates are visited in ascending
// lane order, the visiting lane taken in scalar code from the ballot of the valid lanes: every
// lane runs the same arithmetic on the same values in the same order as rank_candidates does on
// the packed layout, and tau and s_cand come out bitwise the same.
template <int NW>
__device__ __forceinline__ double rank_candidates_express(double mine, uint32_t cnt, uint32_t rr,
                                                          int lane, double* s_cand) {
  constexpr int E = kWave / NW;
  const bool valid = static_cast<uint32_t>(lane & (E - 1)) < cnt;
  unsigned long long m = __ballot(valid);
  RankTally t;
  while (m != 0ull) visit_candidate(mine, m, t);  // uniform
  return ranked_candidate(mine, valid, t, rr, s_cand);
}

// rank_candidates_express with the tail's wave sum (*s_below = the sum of `tail` over the wave, by
// wave_reduce's tree) in the same basic block as the ranking's first candidate: the bucket of this
// path holds at least one, so the first visit is straight-line code whose readlanes and compares
// fill the wait states of the reduction's DPP stages; the loop takes the remaining candidates (the
// usual bucket has none: its exit is the fall-through).  The visits and the end are
// rank_candidates_express's own: tau and s_cand are bitwise the same.
template <int NW>
__device__ __forceinline__ double rank_candidates_express_tail(double mine, uint32_t cnt,
                                                               uint32_t rr, int lane, double tail,
                                                               double* s_below, double* s_cand) {
  constexpr int E = kWave / NW;
  const bool valid = static_cast<uint32_t>(lane & (E - 1)) < cnt;
  unsigned long long m = __ballot(valid);
  RankTally t;
  visit_candidate(mine, m, t);  // the first candidate (m != 0 on this path)
  *s_below = wave_reduce<OpAdd>(tail);
  if (m != 0ull) [[unlikely]] {
    do {  // uniform
      visit_candidate(mine, m, t);
    } while (m != 0ull);
  }
  return ranked_candidate(mine, valid, t, rr, s_cand);
}

// Wave 0 (all lanes active): tau = the candidate of rank rr among the c <= kCap candidates held in
// per-wave regions cand[w * kCap + i], i < wcount[w] (global order: wave, then position — fixed).
// Candidates are pulled into registers (g = lane, lane + 64) and compared through readlane, so
// the O(c^2) ranking never waits on LDS.  Also returns s_cand = sum over candidates below tau of
// (cand - tau), accumulated in candidate order.  Q = candidate registers per lane: 1 when
// c <= 64 (the usual case), 2 up to kCap.
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
  // per candidate v (lane-parallel): #{z < v}, #{z == v} and sum_{z < v} (z - v); the lane of
  // tau then holds s_cand itself, so no reduction follows the ranking
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

// ---------------------------------------------------------------------------------------------
// the exact fallback
// ---------------------------------------------------------------------------------------------
// A source hands select_exact the projections d_i of one unit, this thread's share of them, through
// two visitors: each_sample(f) calls f(d) for the samples this thread holds (any trip count), and
// each_slot(f) calls f(d) the same number of times in every thread of the workgroup, with NaN for a
// slot that holds no sample (never in range, never below: ballots see whole waves).
//
// The unit's samples in memory, re-read (L2/MALL-hot) on every pass: thread `tid` holds samples
// tid, tid + BLOCK, ...; proj(i) is the projection h . xi_i of sample i.
template <int BLOCK, class Proj>
struct MemorySource {
  const Proj& proj;
  int n;
  template <class F>
  __device__ __forceinline__ void each_sample(F&& f) const {
    for (int i = threadIdx.x; i < n; i += BLOCK) f(proj(i));
  }
  template <class F>
  __device__ __forceinline__ void each_slot(F&& f) const {
    for (int i0 = 0; i0 < n; i0 += BLOCK) {  // uniform trip count
      const int i = i0 + static_cast<int>(threadIdx.x);
      f(i < n ? proj(i) : NAN);
    }
  }
};
template <int BLOCK, class Proj>
__device__ __forceinline__ MemorySource<BLOCK, Proj> memory_source(const Proj& proj, int n) {
  return MemorySource<BLOCK, Proj>{proj, n};
}

// The unit's projections held in registers: d[0..Q), bit q of vmask set where slot q holds a
// sample.  Nothing is re-read; an idle slot is NaN to both visitors.
template <int Q>
struct RegisterSource {
  const double (&d)[Q];
  uint32_t vmask;
  template <class F>
  __device__ __forceinline__ void each_slot(F&& f) const {
#pragma unroll
    for (int q = 0; q < Q; ++q) f(((vmask >> q) & 1u) ? d[q] : NAN);
  }
  template <class F>
  __device__ __forceinline__ void each_sample(F&& f) const {
    each_slot(f);
  }
};

// Exact selection for the units the window fast path does not finish (a target outside the window,
// degenerate moments, or a first-pass bucket with more than kCap samples): exact min/max of the
// source's projections, then histogram refinement (value-linear, then order-preserving integer
// keys) until <= kCap candidates remain or the run collapses to one value.  Begins with a barrier
// (the fast path's readers of hist / red_* are done); every wave returns; the result is valid in
// wave 0: tau and dsum = sum_{d<tau} (d - tau).
template <int BLOCK, int LOG_NB, class Source>
__device__ __forceinline__ void select_exact(const Source& src, double mu_d, uint32_t rank,
                                             uint32_t* hist, double* cand, uint32_t* wcount,
                                             double* red_rng, double* red_tail, double* tau_out,
                                             double* dsum_out) {
  constexpr int NW = BLOCK / kWave;
  constexpr int NB = 1 << LOG_NB;
  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int wave = tid / kWave;
  __syncthreads();

  double vmin[1] = {INFINITY}, vmax[1] = {-INFINITY};
  src.each_sample([&](double v) {
    vmin[0] = fmin(vmin[0], v);
    vmax[0] = fmax(vmax[0], v);
  });
  block_reduce<OpMin, NW, 1>(vmin, red_rng);
  block_reduce<OpMax, NW, 1>(vmax, red_rng + NW);
  double lo = vmin[0], hi = vmax[0];
  if (lo == hi) {  // every sample projects to one value (the noise-free step 0): no tail below it
    *tau_out = lo;
    *dsum_out = 0.0;
    return;        // uniform; no second pass over the samples
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
    src.each_sample([&](double v) {
      if (in_range(v, lo, hi)) atomicAdd(&hist[hist_slot<NB>(map(v))], 1u);
    });
    __syncthreads();
    const ScanResult sr = scan_bins<NB>(hist, rr, lane);
    bin = sr.bin;
    rr -= sr.below;
    c = sr.cnt;
    have_bin = true;
    if (c <= kCap) break;
    double rmin[1] = {INFINITY}, rmax[1] = {-INFINITY};
    src.each_sample([&](double v) {
      if (in_range(v, lo, hi) && map(v) == bin) {
        rmin[0] = fmin(rmin[0], v);
        rmax[0] = fmax(rmax[0], v);
      }
    });
    __syncthreads();  // all waves have scanned hist before it is cleared again
    block_reduce<OpMin, NW, 1>(rmin, red_rng);
    block_reduce<OpMax, NW, 1>(rmax, red_rng + NW);
    lo = rmin[0];
    hi = rmax[0];
    have_bin = false;
    if (lo == hi) {
      tau_known = true;
      tau = lo;
    }
  }

  double sq = 0.0;
  uint32_t wbase = 0;
  const unsigned long long lt_mask = (1ull << lane) - 1ull;
  src.each_slot([&](double v) {
    const bool inr = in_range(v, lo, hi);
    const int bj = (have_bin && inr) ? map(v) : 0;
    const bool below = v < lo || (have_bin && inr && bj < bin);
    if (below) sq += v - mu_d;
    append_candidate(cand + wave * kCap, wbase, !tau_known && inr && (!have_bin || bj == bin), v,
                     lt_mask);
  });
  sq = wave_reduce<OpAdd>(sq);
  if (lane == 0) {
    red_tail[wave] = sq;
    wcount[wave] = wbase;
  }
  __syncthreads();
  if (wave != 0) return;
  const double s_below = sum_partials<NW>(red_tail);
  double s_cand = 0.0;
  // lane w < NW: the candidate count of wave w (0 elsewhere)
  if (!tau_known)
    tau = rank_candidates<NW>(cand, lane < NW ? wcount[lane] : 0u, c, rr, lane, &s_cand);
  const double n_below = static_cast<double>(rank - rr);
  *tau_out = tau;
  *dsum_out = (s_below - n_below * (tau - mu_d)) + s_cand;
}

// compute_separating_vector(ego, mu) (core/geometry.py:35-53): (mu - ego) / |mu - ego|, [1, 0]
// below 1e-10.  RSQRT is the kernel's reciprocal square root — rsqrt_nr for the stored form,
// rsqrt_nr2 for the sampled one: the two give different bits of h on purpose, and each kernel's
// tests hold it to its own.  Branch-free: an overflowing norm (n2 = inf) selects 1/inf = 0, as
// diff / norm gives 0 (finite diff) or NaN (infinite diff); a NaN n2 stays NaN.
template <double (*RSQRT)(double)>
__device__ __forceinline__ void separating_direction(double mux, double muy, double e0, double e1,
                                                     double deg_sq, double* h0, double* h1) {
  const double dx = mux - e0, dy = muy - e1;
  const double n2 = dx * dx + dy * dy;
  const double inv = n2 == INFINITY ? 0.0 : RSQRT(n2);
  const bool degenerate = n2 < deg_sq;
  *h0 = degenerate ? 1.0 : dx * inv;
  *h1 = degenerate ? 0.0 : dy * inv;
}

// |h| for R_c |h| (risk_metrics.py:293, :234).  h is a unit vector up to rounding on the
// separating-direction path, where sqrt(1 + e) = 1 + e/2 - e^2/8 (+ O(e^3)) replaces the long
// fp64 sqrt sequence (e = |h|^2 - 1 is exact there; the result is within 1 ulp of the correctly
// rounded sqrt — it can differ only where 1 + e/2 is a rounding tie); any other h takes sqrt.
__device__ __forceinline__ double norm_h(double h0, double h1) {
  const double n2 = h0 * h0 + h1 * h1;
  const double e = n2 - 1.0;
  if (fabs(e) < 0x1p-40) return 1.0 + fma(-0.125 * e, e, 0.5 * e);  // uniform branch
  return sqrt(n2);
}

// Per-unit status word (DRCVAR_UNIT_*): which of the reference's solver-failure branches the unit
// took (core/risk_metrics.py:173-177,261-265: the LP status; :298-303,334-338: the sentinels) —
// reported by the kernel itself, so no caller has to infer it from the sentinel's value.
__device__ __forceinline__ int32_t failure_status(bool nonfinite, const Params& prm) {
  return (nonfinite ? DRCVAR_UNIT_NONFINITE : 0) | (prm.unbounded ? DRCVAR_UNIT_UNBOUNDED : 0) |
         (prm.epsilon < 0.0 ? DRCVAR_UNIT_DR_UNBOUNDED : 0);
}

// Columns 5..7 of the record from the lower-tail statistics: L = tau + dsum / k is the lower-tail
// mean, r = R_c |h| (risk_metrics.py:293, :234).
struct Offsets {
  double g_cvar, g_star, g_tilde;
};
__device__ __forceinline__ Offsets offsets_from_tail(const Params& prm, double r, double tau,
                                                     double dsum) {
  const double L = tau + dsum * prm.inv_k;
  Offsets g{r - prm.delta - L, kSentinel, kSentinel - r};
  if (prm.epsilon >= 0.0) {  // else: DR LP unbounded (lambda -> inf), solver-failure sentinel
    g.g_star = r - prm.delta + prm.eps_over_alpha - L;
    g.g_tilde = g.g_star - r;
  }
  return g;
}
// ... and of a unit whose solve failed (risk_metrics.py:298-303,334-338); its status word is
// failure_status's.
__device__ __forceinline__ Offsets failure_offsets(double r) {
  return Offsets{kSentinel, kSentinel, kSentinel - r};
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// Standard-normal quantile (P. J. Acklam's rational approximation, |rel err| < 1.2e-9) — only
// positions the fast-path window, so its accuracy never affects results.
inline double normal_quantile(double p) {
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

// Everything of Params that depends on the call alone; inv_n0 and hist_scale depend on the launch
// plan and are set there (0 until then).
inline Params make_params(double rr, double ro, double alpha, double delta, double eps, int64_t n) {
  Params p{};
  p.rc = rr + ro;
  p.alpha = alpha;
  p.delta = delta;
  p.epsilon = eps;
  p.eps_over_alpha = eps / alpha;
  const double dn = static_cast<double>(n);
  p.inv_n = 1.0 / dn;
  p.k = alpha * dn;                      // exactly as the reference forms alpha * n_samples
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

inline bool params_ok(double rr, double ro, double alpha, double delta, double eps) {
  return std::isfinite(rr) && std::isfinite(ro) && std::isfinite(alpha) && alpha > 0.0 &&
         std::isfinite(delta) && std::isfinite(eps);
}
