// drcvar_generator.inc — the obstacle-sample generator's device arithmetic (Philox4x32-10,
// Box-Muller from 32-bit uniforms, the LDS tables, the pair of samples of one Philox call) and the
// uniforms it takes (PhiloxUniform, LogScale; host-made, PhiloxUniform also in scalar device
// code), for the three kernels that draw: the
// sampler (drcvar_sampling.hip), the clearance evaluation (drcvar_clearance.hip) and the sampled
// halfspaces (drcvar_sampled.hip).  Included inside each file's anonymous namespace, after
// <cstdint> and <cstring>.  The host mirror is oracle/philox_sampler.py.

#include "drcvar_sampling_tables.inc"

struct Philox {
  uint32_t x[4];
};

// Philox4x32-10 on the counter (c0, c1, s0, s1): c0, c1 vary per lane, the stream words s0, s1 and
// the key (k0, k1) are uniform, so the first round's M1 s0 and every xor of uniform words are made
// once on the host (PhiloxUniform): round 1 costs one v_mad_u64_u32 and two v_xor_b32, round 2 two
// products, a v_xor with a scalar operand and one v_bitop3 (the asm form below copied each uniform
// word to a VGPR first: one v_mov per word and call).
struct PhiloxUniform {
  uint32_t a1;  // hi(M1 s0) ^ k0: round 1's new c0 is c1 ^ a1
  uint32_t b1;  // lo(M1 s0): round 1's new c1
  uint32_t c1;  // s1 ^ k1: round 1's new c2 is hi(M0 c0) ^ c1
  uint32_t b2;  // b1 ^ (k0 + W0): round 2's new c0 is hi(M1 c2) ^ b2
  uint32_t k0, k1;
};

constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
constexpr uint64_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;

// (Host and device: the device-state form of the sampled halfspaces makes it in the kernel, in
// scalar code, from stream words it loads; every other kernel takes the host-made struct.)
__host__ __device__ inline PhiloxUniform make_philox_uniform(uint32_t s0, uint32_t s1, uint32_t k0,
                                                             uint32_t k1) {
  const uint64_t q1 = kPhiloxM1 * s0;
  PhiloxUniform p{};
  p.a1 = static_cast<uint32_t>(q1 >> 32) ^ k0;
  p.b1 = static_cast<uint32_t>(q1);
  p.c1 = s1 ^ k1;
  p.b2 = p.b1 ^ (k0 + kPhiloxW0);
  p.k0 = k0;
  p.k1 = k1;
  return p;
}

__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, const PhiloxUniform& pu) {
  constexpr uint64_t kM0 = kPhiloxM0, kM1 = kPhiloxM1;
  constexpr uint32_t kW0 = kPhiloxW0, kW1 = kPhiloxW1;
  uint32_t k0 = pu.k0 + kW0, k1 = pu.k1 + kW1;  // round 2's keys (SALU)
  // round 1: (c0, c1, s0, s1) -> (hi(M1 s0) ^ c1 ^ k0, lo(M1 s0), hi(M0 c0) ^ s1 ^ k1, lo(M0 c0))
  const uint64_t q0 = kM0 * c0;
  c0 = c1 ^ pu.a1;
  uint32_t c2 = static_cast<uint32_t>(q0 >> 32) ^ pu.c1;
  uint32_t c3 = static_cast<uint32_t>(q0);
  // round 2 (c1 = b1 uniform)
  {
    const uint64_t p0 = kM0 * c0, p1 = kM1 * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ pu.b2;
    uint32_t n2;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(n2) : "v"(static_cast<uint32_t>(p0 >> 32)), "v"(c3), "s"(k1));
    c0 = n0;
    c1 = static_cast<uint32_t>(p1);
    c2 = n2;
    c3 = static_cast<uint32_t>(p0);
  }
#pragma unroll
  for (int r = 2; r < 10; ++r) {
    // The key schedule is bumped in SALU each round (volatile: otherwise all twenty round keys are
    // hoisted out of the sample loop, spilled to VGPR lanes and read back with one v_readlane per
    // use — VALU work in a VALU-bound kernel).
    asm volatile("s_add_u32 %0, %0, %1" : "+s"(k0) : "s"(kW0) : "scc");
    asm volatile("s_add_u32 %0, %0, %1" : "+s"(k1) : "s"(kW1) : "scc");
    const uint64_t p0 = kM0 * c0, p1 = kM1 * c2;  // one v_mad_u64_u32 each
    uint32_t n0, n2;  // hi(p1) ^ c1 ^ k0, hi(p0) ^ c3 ^ k1 (the key words are uniform: SGPRs)
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(n0) : "v"(static_cast<uint32_t>(p1 >> 32)), "v"(c1), "s"(k0));
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(n2) : "v"(static_cast<uint32_t>(p0 >> 32)), "v"(c3), "s"(k1));
    c0 = n0;
    c1 = static_cast<uint32_t>(p1);
    c2 = n2;
    c3 = static_cast<uint32_t>(p0);
  }
  return Philox{{c0, c1, c2, c3}};
}

// fma with a uniform third operand held in SGPRs (the polynomial coefficients): as v_fma_f64 with
// an SGPR source instead of the compiler's v_mov_b64 of a VGPR-held coefficient + v_fmac_f64 —
// one VALU instruction per Horner step instead of two.  Same IEEE fma, same bits.
__device__ __forceinline__ double fma_sc(double a, double b, double c) {
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
  return r;
}

// a b + c with the uniform b in SGPRs.
__device__ __forceinline__ double fma_vs(double a, double b, double c) {
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b), "v"(c));
  return r;
}

// The scale of the log: the sampler computes y = lam (-2 log u), lam = l^2 for an isotropic
// covariance l^2 I (the reference's default diag(0.01, 0.01), simulation/obstacles.py:134), so that
// sqrt(y) is already the scaled radius and a sample is nominal + sqrt(y) (cos, sin): two fmas
// instead of the two products and three fmas of nominal + L z.  lam = 1 otherwise.  Host-made:
//   q[0..4]  lam times the coefficients of -P/2 (below), Horner order
//   eh, el   -2 lam ln 2 split so that e * eh is exact for |e| <= 33 (eh: 46 significant bits)
struct LogScale {
  double lam, q0, q1, q2, q3, q4, eh, el;
};

// LogScale for lam: the Horner coefficients of -P/2 in r2 (1/192, 1/80, 1/32, 1/12, 1/4) times
// lam, and -2 lam ln 2 split into a 46-bit head (e * eh exact for |e| <= 33) and a tail, from an
// extended-precision product.
inline LogScale make_log_scale(double lam) {
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

// lam (-2 log u) for the uniform u = (x + 1/2) 2^-32 in the open interval (0, 1) of a 32-bit word
// (at most 33 significant bits: exact, in [2^-33, 1 - 2^-33], never 0 or 1).  It is formed as
// w = 2x + 1 (one fma with inline constants, exact) and u = w 2^-33, folded into the exponent.
// u = m 2^e, m in [1/2, 1); the top 9 mantissa bits, rounded, pick the nearest centre
// c_k = 1/2 + k/512 (k = 0..256; c_256 = 1 exactly, so log u keeps its relative accuracy as u -> 1);
// r2 = -2 r = 2 - 2 m (1/c_k) by one fma from the LDS entry -2/c_k (|r| <= 1/512 + 2^-52; exact
// table and constant, so the cancellation costs nothing); -2 log m = 2 log(1/c_k) - 2 log1p(r) and
// -2 log1p(r) = r2 + r2^2 (-P(r)/2), P to r^4 (the next term, r^7 / 7, is below 2^-56 of r), the
// Horner coefficients those of -P/2 in r2.  Scaled: lam (r2 + r2^2 q) = r2 fma(r2, lam q, lam)
// (the same two instructions as r2 + r2^2 q), lam q by the lam-scaled coefficients, and the LDS
// table's second entry is lam 2 log(1/c_k) (scaled when the table is copied).  With lam = 1 every
// scaled value is the unscaled one.
__device__ __forceinline__ double scaled_neg2_log_u32(uint32_t x, const double* log_t,
                                                      const LogScale& c) {
  const double w = fma(static_cast<double>(x), 2.0, 1.0);
  const double m = __builtin_amdgcn_frexp_mant(w);
  const int e = __builtin_amdgcn_frexp_exp(w) - 33;
  const uint32_t idx = __builtin_amdgcn_ubfe(static_cast<uint32_t>(__double2hiint(m)), 11, 9);
  const double ninv2 = log_t[2 * idx], log_inv2 = log_t[2 * idx + 1];  // -2/c_k, lam 2 log(1/c_k)
  const double r2 = fma(m, ninv2, 2.0);                                 // -2 r
  double q = fma(r2, c.q0, c.q1);
  q = fma_sc(q, r2, c.q2);
  q = fma_sc(q, r2, c.q3);
  q = fma_sc(q, r2, c.q4);                                              // lam (-P(r) / 2)
  const double m2log1p = r2 * fma_sc(r2, q, c.lam);                     // lam (-2 log1p(r))
  const double de = static_cast<double>(e);
  return fma_vs(de, c.eh, fma_vs(de, c.el, log_inv2 + m2log1p));
}

// sqrt(y).  The argument is >= lam 2^-33 ln 4 > 0, never denormal (lam >= 2^-200, host-checked),
// so rsq + two Newton-Raphson steps (Goldschmidt form) replace the library sqrt and its rescaling.
__device__ __forceinline__ double sqrt_normal(double y) {
  const double rs = __builtin_amdgcn_rsq(y);
  double h = 0.5 * rs, r = y * rs;
  const double e = fma(-r, h, 0.5);
  r = fma(r, e, r);
  h = fma(h, e, h);
  return fma(fma(-r, r, y), h, r);
}

// (cos, sin)(2 pi w / 2^32): table point k = round(w / 2^23) mod 512 (32-bit wrap-around), signed
// remainder rem = w - k 2^23 in [-2^22, 2^22), b = 2 pi rem / 2^32 in [-pi/512, pi/512);
// sin b = b + b^3 (-1/6 + b^2/120) (next term b^7/5040: 1e-17 of b), cos b - 1 = b^2 (-1/2 + b^2/24)
// (next term b^6/720 < 8e-17), and (cos, sin)(a + b) = (C (1 + cm1) - S sb, S (1 + cm1) + C sb)
// with (C, S) = kTurn[k].  (-0.5 is an inline constant: fma(z, 1/24, -0.5) needs no VGPR copy of
// either coefficient.)
__device__ __forceinline__ void cos_sin_u32(uint32_t w, const double* turn, double* cs, double* sn) {
  const uint32_t k = (w + (1u << 22)) >> 23;
  const int32_t rem = __builtin_amdgcn_sbfe(static_cast<int32_t>(w), 0, 23);  // = w - k 2^23
  constexpr double kTurn32 = 6.28318530717958647692 * 0x1.0p-32;
  const double b = static_cast<double>(rem) * kTurn32;
  const double z = b * b;
  const double ps = fma(z, 1.0 / 120.0, -1.0 / 6.0);
  const double sb = fma(b * z, ps, b);
  const double cm1 = z * fma(z, 1.0 / 24.0, -0.5);
  const double C = turn[2 * k], S = turn[2 * k + 1];
  *cs = fma(C, cm1, fma(-S, sb, C));
  *sn = fma(S, cm1, fma(C, sb, S));
}

// The pair of samples of one Philox call (counter g, the unit's nominal point): sample p from the
// call's first (radius, angle) words, sample p + P from its second.  kIso: the covariance is l^2 I
// and the log already carries lam = l^2 (LogScale), so a sample is nominal + radius (cos, sin);
// otherwise nominal + L z as an fma chain (the mirror rounds ny + (l10 z0 + l11 z1): a few ulp apart).
// Args: the kernel's argument struct, with the Cholesky entries l00, l10, l11, pu and lg.
template <bool kIso, class Args>
__device__ __forceinline__ void draw_pair(uint64_t g, const Args& a, double nx, double ny,
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

constexpr int kTurnLen = sizeof(kTurn) / sizeof(double);
constexpr int kLogIdx = 2 * (sizeof(kLogT) / sizeof(double) / 2 - 1);  // 512 nine-bit indices
constexpr int kGenTableDoubles = kTurnLen + 2 * kLogIdx;               // LDS the tables take

// The tables into LDS (s_turn [kTurnLen], s_log [2 kLogIdx]) by `threads` threads, the log's
// second column scaled by lam; the caller synchronises before the first use.
__device__ __forceinline__ void load_generator_tables(double* s_turn, double* s_log, int threads,
                                                      double lam) {
  for (int i = threadIdx.x; i < kTurnLen + kLogIdx; i += threads) {
    if (i < kTurnLen) {
      s_turn[i] = kTurn[i];
    } else {  // index j -> centre (j + 1) / 2, scaled by -2 (exact)
      const int j = i - kTurnLen, c = (j + 1) >> 1;
      s_log[2 * j] = -2.0 * kLogT[2 * c];
      s_log[2 * j + 1] = lam * (-2.0 * kLogT[2 * c + 1]);
    }
  }
}
