"""High-precision reference, error bound, mutations, case table and window mirror for the fused
halfspace kernel (csrc/drcvar_halfspace.hip).  A helper of tests/test_halfspace_reference.py (CPU)
and tests/test_halfspace_selection.py (GPU): plain NumPy, never the product path, and it does not
import the engine.

Reference
---------
``reference(samples, ego=..., h=...)`` evaluates a block of units ``samples [U, N, 2]`` with the
formulas of oracle/closed_form.py (separating vector with its ``[1, 0]`` fallback below 1e-10, mean
halfspace from the origin, ``L = (sum_{j<m} d_(j) + (k - m) d_(m)) / k`` over a FULL sort, the
sentinels of the solver-failure branches), every sum and projection in ``np.longdouble`` (64-bit
mantissa here: 2^11 times finer than the fp64 it is compared with).  ``k = alpha * N`` is formed in
fp64 exactly as the kernel's host code and the Python original form it.

Error bound
-----------
``Ref.bound`` is the tolerance of every tight comparison of an offset (g_cvar, g_star, g_tilde)
with the reference.  With u = 2^-53, b = #{d < tau} and rho = |mu - ego| it is the sum of

* summation, ``(min(N, b + 128) + 2) u S / k`` with ``S = sum_{d<tau} (|d - mu_d| + |tau - mu_d|)``:
  the kernel forms ``dsum = sum_{below}(d - mu_d) - b (tau - mu_d) + sum_{cand<tau}(z - tau)`` in an
  order of its own; any order of n fp64 additions is within ``(n - 1) u`` of the absolute sum of its
  terms, the terms are rounded once each, the product ``b (tau - mu_d)`` twice; at most b terms lie
  below the target bucket and at most kCap = 128 candidates are ranked.  ``L = tau + dsum / k``.
* projection, ``2 u max_i(|h0 x_i| + |h1 y_i|) + dh max_i(|x_i| + |y_i|)``: L is 1-Lipschitz in
  ``max_i |delta d_i|``; ``fma(h0, x, h1 y)`` rounds twice; ``dh`` is how far the kernel's own h may
  lie from the reference's: 0 when h is given; else ``4 u + (dmu_x + dmu_y) / rho`` — normalising
  v = mu - ego is 1/rho-Lipschitz, the subtraction, the rsqrt (hardware seed + one Newton step,
  ~1 ulp) and the product round once each, and the mean the kernel sums in fp64 in any order is
  within ``dmu = N u mean|x|`` (per coordinate) of the exact mean.  (This last term is the one the
  issue's sketch did not list; without it h cannot be compared at all at N = 40 000.)
* final arithmetic, ``4 u (|tau| + |L| + R_c |h| + |delta| + |eps / alpha|) + 2 u |L - tau|``.

``Ref.bound_h`` (= dh, at least 4 u), ``Ref.bound_hm`` and ``Ref.bound_gm`` are the matching bounds
of the direction, the mean direction and the mean offset.  The pivot mu_d needs no term: dsum is
algebraically independent of it.

Mutations (CPU only: they show that a comparison at the bound can fail)
-----------------------------------------------------------------------
``mutated_g_cvar(ref, i, kind)``: ``rank_lo`` / ``rank_hi`` — tau taken from rank m - 1 / m + 1 with a
consistent tail sum; ``drop`` — the tail sample nearest tau left out of sum_{d<tau}(d - tau);
``le`` — one sample equal to tau counted below it, ``<=`` for ``<``: it enters the kernel's sum
of (d - mu_d) below the bucket while the count below stays (the consistent variants of this fault
are no-ops, a tie contributes (tau - tau) = 0).

Case table and window mirror: see ``cases`` and ``predict_path``.
"""
import math
from dataclasses import dataclass

import numpy as np

LD = np.longdouble
U64 = 2.0 ** -53
SENTINEL = 100.0
RR, RO, DELTA, EPSILON = 0.3, 0.3, 0.1, 0.15
K_CAP = 128

# (threads, samples per thread, log2 bins) of every compiled launch geometry; the first ten are the
# automatic chain (smallest with threads * per >= N)
GEOMETRIES = [(64, 2, 7), (128, 4, 8), (256, 4, 9), (256, 8, 10), (256, 16, 10), (256, 20, 10),
              (512, 16, 10), (512, 20, 10), (1024, 12, 10), (1024, 16, 10),
              (64, 16, 9), (128, 8, 9), (512, 2, 9), (1024, 10, 10)]
N_AUTOMATIC = 10
STREAM_BLOCK = 1024
STREAM_SIZES = [16385, 40000]
A0 = (0.0, 0.02, 0.2, 0.5, 0.9, 1.0)     # alpha classes


def sizes_of(block, per):
    """The sizes a geometry is tested at: full, one into the last row, one past / short of row 0
    (and the tiny ones on the smallest plan)."""
    s = [block * per, block * (per - 1) + 1, block + 1, block - 1]
    if (block, per) == (64, 2):
        s += [1, 2, 3, 64]           # 63 and 65 are block -+ 1 already
    return s


def head_of(block, per):
    """Size of the subsample the kernel places its window from: the 64-sample pilot on plans with
    per <= 8, row 0 (the first `block` samples) otherwise."""
    return 64 if per <= 8 else block


def automatic_geometry(n):
    for g in GEOMETRIES[:N_AUTOMATIC]:
        if n <= g[0] * g[1]:
            return g
    return None   # streaming kernel


def alpha_of(n, a0):
    """(alpha, m): m = floor(a0 N) clipped to N - 1, alpha = (m + 0.5) / N, so that the weight
    k - m of tau in L is about one half in every class (a0 = 0: k < 1; a0 = 1: tau = max)."""
    m = min(int(math.floor(a0 * n)), n - 1)
    alpha = (m + 0.5) / n
    assert int(math.floor(alpha * n)) == m and alpha * n <= n
    return alpha, m


# ---------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------
@dataclass
class Ref:
    rec: np.ndarray        # [U, 8] fp64 (rounded from long double)
    tau: np.ndarray        # [U] long double
    L: np.ndarray
    mu_d: np.ndarray
    d_sorted: np.ndarray   # [U, N] long double
    m: int
    k: float
    alpha: float
    bound: np.ndarray      # [U] offsets g_cvar, g_star, g_tilde
    bound_h: np.ndarray    # [U] each component of h
    bound_hm: np.ndarray   # [U] each component of the mean direction
    bound_gm: np.ndarray   # [U] g_mean
    ok: np.ndarray         # [U] no solver-failure branch taken for g_cvar
    n_eq: np.ndarray       # [U] samples equal to tau
    n_below: np.ndarray    # [U] samples strictly below tau


def _sepvec(diff):
    norm = np.sqrt(diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1])
    deg = norm < LD(1e-10)
    with np.errstate(invalid="ignore", divide="ignore"):
        h = diff / norm[..., None]
    h[deg] = (1.0, 0.0)
    return h, norm, deg


def reference(samples, ego=None, h=None, alpha=0.2, delta=DELTA, epsilon=EPSILON, rr=RR, ro=RO):
    """samples [U, N, 2] fp64; ego [U, 2] (safe_halfspaces: one ego per unit) or h [U, 2]
    (offsets_given_h).  -> Ref."""
    s = np.asarray(samples, dtype=np.float64).astype(LD)
    U, N, _ = s.shape
    given = h is not None
    rc = LD(rr) + LD(ro)
    with np.errstate(invalid="ignore", over="ignore"):
        mu = s.sum(axis=1) / LD(N)
        hm, mu_norm, _ = _sepvec(mu)
        hm_norm = np.sqrt(hm[:, 0] ** 2 + hm[:, 1] ** 2)
        g_mean = -((hm[:, 0] * mu[:, 0] + hm[:, 1] * mu[:, 1]) - rc * hm_norm)
        if given:
            hh = np.asarray(h, dtype=np.float64).astype(LD)
            rho = np.full(U, np.inf, dtype=LD)
            deg = np.ones(U, dtype=bool)
        else:
            hh, rho, deg = _sepvec(mu - np.asarray(ego, dtype=np.float64).astype(LD))
        hn = np.sqrt(hh[:, 0] ** 2 + hh[:, 1] ** 2)
        r = rc * hn
        finite = np.isfinite(np.asarray(samples, dtype=np.float64)).all(axis=(1, 2))
        d = hh[:, None, 0] * s[:, :, 0] + hh[:, None, 1] * s[:, :, 1]
        d = np.where(finite[:, None], d, LD(0))
        mu_d = np.where(finite, hh[:, 0] * mu[:, 0] + hh[:, 1] * mu[:, 1], LD(0))
    k = float(alpha) * float(N)                      # fp64, as the kernel's host code forms it
    unbounded = not (k <= N)
    ds = np.sort(d, axis=1)
    if unbounded:
        m, idx = 0, 0
        tau = ds[:, 0]
        L = np.full(U, np.nan, dtype=LD)
    else:
        m = int(math.floor(k))
        idx = min(m, N - 1)
        tau = ds[:, idx]
        L = (ds[:, :m].sum(axis=1) + (LD(k) - LD(m)) * tau) / LD(k)
    ok = finite & (not unbounded)
    with np.errstate(invalid="ignore"):
        g_cvar = np.where(ok, r - LD(delta) - L, LD(SENTINEL))
        g_star = np.where(ok & (epsilon >= 0.0), r - LD(delta) + LD(epsilon) / LD(alpha) - L,
                          LD(SENTINEL))
        g_tilde = g_star - r
    rec = np.empty((U, 8), dtype=np.float64)
    rec[:, 0:2], rec[:, 2], rec[:, 3:5] = hm, g_mean, hh
    rec[:, 5], rec[:, 6], rec[:, 7] = g_cvar, g_star, g_tilde

    # ---- bound (module docstring) ----
    a = np.abs(np.asarray(samples, dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        dmu = N * U64 * a.mean(axis=1)                                    # [U, 2]
        dmu_sum = dmu[:, 0] + dmu[:, 1]
        dh = np.where(deg, 0.0, 4 * U64 + dmu_sum / np.maximum(rho.astype(np.float64), 1e-300))
        h64 = np.abs(hh.astype(np.float64))
        e_proj = (2 * U64 * (h64[:, None, 0] * a[:, :, 0] + h64[:, None, 1] * a[:, :, 1]).max(axis=1)
                  + dh * (a[:, :, 0] + a[:, :, 1]).max(axis=1))
        below = ds < tau[:, None]
        n_below = below.sum(axis=1)
        S = (np.where(below, np.abs(ds - mu_d[:, None]), 0).sum(axis=1)
             + n_below * np.abs(tau - mu_d)).astype(np.float64)
        e_sum = (np.minimum(N, n_below + K_CAP) + 2) * U64 * S / k
        Lf = np.nan_to_num(L.astype(np.float64))
        tf = tau.astype(np.float64)
        e_fin = 4 * U64 * (np.abs(tf) + np.abs(Lf) + float(rc) * hn.astype(np.float64) + abs(delta)
                           + abs(epsilon / alpha)) + 2 * U64 * np.abs(Lf - tf)
        bound = e_proj + e_sum + e_fin
        bound_hm = 4 * U64 + np.where(mu_norm < 1e-10, 0.0,
                                      dmu_sum / np.maximum(mu_norm.astype(np.float64), 1e-300))
        bound_gm = dmu_sum + 4 * U64 * (np.abs(mu.astype(np.float64)).sum(axis=1) + float(rc))
    return Ref(rec, tau, L, mu_d, ds, m, k, float(alpha), bound, np.maximum(dh, 4 * U64), bound_hm,
               bound_gm, ok, (ds == tau[:, None]).sum(axis=1), n_below)


def lower_tail(ds, k, r):
    """L with tau taken from rank r of the sorted projections `ds` and a consistent tail sum."""
    return (ds[:r].sum() + (LD(k) - LD(r)) * ds[r]) / LD(k)


MUTATIONS = ("rank_lo", "rank_hi", "drop", "le")


def mutated_g_cvar(ref, i, kind):
    """g_cvar of unit i under one seeded mistake, or None where the mistake does not apply (no such
    rank; no sample strictly below tau; tau not tied, or all samples one value)."""
    ds, k = ref.d_sorted[i], ref.k
    n = len(ds)
    idx = min(ref.m, n - 1)
    tau, L = ref.tau[i], ref.L[i]
    if kind == "rank_lo":
        if idx - 1 < 0:
            return None
        Lm = lower_tail(ds, k, idx - 1)
    elif kind == "rank_hi":
        if idx + 1 > n - 1:
            return None
        Lm = lower_tail(ds, k, idx + 1)
    elif kind == "drop":
        b = int(ref.n_below[i])
        if b < 1:
            return None
        Lm = L - (ds[b - 1] - tau) / LD(k)
    elif kind == "le":
        if ref.n_eq[i] < 2 or ref.n_eq[i] == n:   # (all one value: tau = mu_d, nothing to see)
            return None
        Lm = L + (tau - ref.mu_d[i]) / LD(k)
    else:
        raise ValueError(kind)
    return float(LD(ref.rec[i, 5]) + (L - Lm))


# ---------------------------------------------------------------------------------------------
# case table
# ---------------------------------------------------------------------------------------------
PLANTED = ("gauss", "bimodal30", "bimodal10", "gauss_asc", "gauss_desc", "head_tight",
           "head_narrow", "head_wide", "head_equal", "gauss_degenerate_dir")
TIES = ("round01", "three_values", "crowd_tau")
# no neighbour of tau that a rank mistake could resolve: every mutation is (nearly) a no-op;
# gauss_plain is the Gaussian WITHOUT the planted gap: on the large plans the gap (wider than a
# histogram bin) leaves tau alone in its bucket, and only an unplanted unit has several candidates
# and a non-zero sum over the candidates below tau
FLAT = ("geometric", "all_equal", "collinear_perp", "novar_exact", "gauss_plain")
FAMILIES = PLANTED + TIES + FLAT
SIGMA = 0.2
RHO = 3.0


def _plant_gap(t, m):
    """Isolate rank m of t: samples above it move up, samples below it down, by 1e-3 of the
    spread.  Samples equal to it stay (exact ties stay exact)."""
    order = np.argsort(t, kind="stable")
    rank = np.empty(len(t), dtype=np.int64)
    rank[order] = np.arange(len(t))
    tm = t[order[m]]
    g = 1e-3 * max(float(np.std(t)), 1e-300)
    t = t.copy()
    t[(rank > m) & (t > tm)] += g
    t[(rank < m) & (t < tm)] -= g
    return t


def _unit(name, n, m, head, rng):
    """(points [n, 2], ego [2]) of one named unit; tau's rank is m."""
    ang = rng.uniform(0, 2 * np.pi)
    hs = np.array([np.cos(ang), np.sin(ang)])
    c = rng.uniform(-3, 3, size=2)
    hd = min(head, n // 2)     # (a head that covered the whole unit would be no head)
    t = rng.normal(size=n) * SIGMA
    s = rng.normal(size=n) * SIGMA
    ego_is_mean = False
    if name in ("gauss", "gauss_plain"):
        pass
    elif name == "gauss_degenerate_dir":
        hs, ego_is_mean = np.array([1.0, 0.0]), True
    elif name in ("bimodal30", "bimodal10"):
        far = rng.random(n) < (0.3 if name == "bimodal30" else 0.1)
        t = t - np.where(far, 20 * SIGMA, 0.0)
    elif name == "gauss_asc":
        o = np.argsort(t)
        t, s = t[o], s[o]
    elif name == "gauss_desc":
        o = np.argsort(-t)
        t, s = t[o], s[o]
    elif name in ("head_tight", "head_narrow"):
        f = 1e-6 if name == "head_tight" else 1e-2
        t[:hd] *= f
        s[:hd] *= f
    elif name == "head_wide":
        t[hd:] *= 1e-6
        s[hd:] *= 1e-6
    elif name == "head_equal":
        # the head away from rank m where the sizes allow it, so that tau stays unique
        t[:hd] = 4 * SIGMA if m < n - hd else -4 * SIGMA
        s[:hd] = 0.5 * SIGMA
    elif name == "round01":      # skewed (median != mean), rounded to a tenth of sigma
        t = np.round(10 * (np.exp(0.5 * rng.normal(size=n)) - 1.0)) * 0.1 * SIGMA
        s = SIGMA * np.sin(37.0 * t / SIGMA)
    elif name == "three_values":
        t = rng.choice([0.0, 1.0, 3.0], size=n, p=[0.5, 0.3, 0.2]) * SIGMA
        s = 0.5 * t
    elif name == "crowd_tau":    # > 128 samples exactly at tau where N allows it, others around
        e = min(n, 200, max(2, (3 * n) // 4))
        lo = int(np.clip(m - e // 2, 0, n - e))
        t = np.concatenate([-0.01 * SIGMA - np.abs(rng.normal(size=lo)) * SIGMA, np.zeros(e),
                            0.01 * SIGMA + np.abs(rng.normal(size=n - lo - e)) * 3 * SIGMA])
        t = t[rng.permutation(n)]
        s = SIGMA * np.sin(37.0 * t / SIGMA)
    elif name == "geometric":    # one candidate eliminated per value-linear pass -> key mode
        t, s, c = 2.0 ** -(np.arange(n) % 900).astype(np.float64), np.zeros(n), np.zeros(2)
    elif name == "all_equal":
        t, s = np.zeros(n), np.zeros(n)
    elif name == "collinear_perp":
        t = np.zeros(n)
    elif name == "novar_exact":
        # direction exactly [1, 0] (ego = mean), the head's x exactly the mean's x (= 0: the rest
        # are +- pairs of small dyadic numbers, whose sums are exact in any order), so every
        # deviation the window's variance is computed from is exactly zero
        hd = min(head, n)
        x = np.zeros(n)
        rest = n - hd
        q = rng.integers(1, 1 << 20, size=rest // 2).astype(np.float64) * 2.0 ** -22
        x[hd:hd + 2 * (rest // 2)] = np.concatenate([q, -q])[rng.permutation(2 * (rest // 2))]
        pts = np.stack([x, rng.normal(size=n) * SIGMA + c[1]], axis=1)
        return pts, pts.mean(axis=0)
    else:
        raise ValueError(name)
    if name in PLANTED:
        t = _plant_gap(t, m)
    pp = np.array([-hs[1], hs[0]])
    pts = c + t[:, None] * hs + s[:, None] * pp
    mean = pts.mean(axis=0)
    return pts, (mean if ego_is_mean else mean - RHO * hs)


_CASES = {}


def cases(n, alpha_class, seed=0, head=64):
    """The block of named units at size n for alpha class `alpha_class` (index into A0):
    dict(names, samples [U, n, 2], ego [U, 2], alpha, m).  `head` = head_of(geometry)."""
    key = (n, alpha_class, seed, head)
    if key not in _CASES:
        alpha, m = alpha_of(n, A0[alpha_class])
        rng = np.random.default_rng([n, alpha_class, seed, head])
        units = [_unit(name, n, m, head, rng) for name in FAMILIES]
        _CASES[key] = dict(names=list(FAMILIES), alpha=alpha, m=m,
                           samples=np.ascontiguousarray(np.stack([u[0] for u in units])),
                           ego=np.ascontiguousarray(np.stack([u[1] for u in units])))
        if len(_CASES) > 12:     # (a block is up to 13 MB; callers walk (n, class) in order)
            _CASES.pop(next(iter(_CASES)))
    return _CASES[key]


GIVEN_H_ONLY = ("h_zero", "h_1e-3", "h_1e3")


def given_h_cases(block):
    """Units of the given-h entry: the block's own units with the reference's h (fp64), then the
    planted Gaussian with h = 0, |h| = 1e-3 and |h| = 1e3.  -> (names, samples, h)."""
    ref = reference(block["samples"], ego=block["ego"], alpha=block["alpha"])
    g = block["names"].index("gauss")
    hg = ref.rec[g, 3:5]
    samples = np.concatenate([block["samples"], np.repeat(block["samples"][g:g + 1], 3, axis=0)])
    h = np.concatenate([ref.rec[:, 3:5], [hg * 0.0, hg * 1e-3, hg * 1e3]])
    return block["names"] + list(GIVEN_H_ONLY), np.ascontiguousarray(samples), np.ascontiguousarray(h)


# ---------------------------------------------------------------------------------------------
# window mirror
# ---------------------------------------------------------------------------------------------
def normal_quantile(p):
    """P. J. Acklam's rational approximation, as the kernel's host code evaluates it."""
    a = (-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02,
         1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00)
    b = (-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02,
         6.680131188771972e+01, -1.328068155288572e+01)
    c = (-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00,
         -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00)
    d = (7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00,
         3.754408661907416e+00)
    p = min(max(p, 1e-12), 1.0 - 1e-12)
    plow = 0.02425
    if p < plow:
        q = math.sqrt(-2.0 * math.log(p))
        return ((((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5])
                / ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1.0))
    if p > 1.0 - plow:
        return -normal_quantile(1.0 - p)
    q = p - 0.5
    r = q * q
    return ((((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q
            / (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0))


def window_params(alpha, n):
    """(z_lo, window_sd, rank) of make_params."""
    a = min(max(alpha, 1e-12), 1.0 - 1e-12)
    z = normal_quantile(a)
    phi = math.exp(-0.5 * z * z) * 0.3989422804014327
    se = math.sqrt(a * (1.0 - a) / n) / phi
    wsd = max(0.25, 12.0 * se)
    m = int(math.floor(alpha * n))
    return z - wsd, wsd, min(m, n - 1)


FAST, BELOW, ABOVE, CROWDED, NOVAR, UNSURE = "FAST", "BELOW", "ABOVE", "CROWDED", "NOVAR", "UNSURE"


def window_variance(pts, h, mu, block, per):
    """The kernel's window variance of one unit: fp32; the 64-sample pilot about the exact mean
    when per <= 8, else the pivot-shifted second moments of row 0.  -> (var_d, noise): `noise` is
    the size below which its sign depends on the order of the fp32 sums."""
    n = len(pts)
    f32 = np.float32
    if per <= 8:
        n0 = min(n, 64)
        d = h[0] * pts[:n0, 0] + h[1] * pts[:n0, 1]
        fm = (d - (h[0] * mu[0] + h[1] * mu[1])).astype(f32)
        s1, s2 = float(fm.sum(dtype=f32)), float((fm * fm).sum(dtype=f32))
        exact = bool(np.all(fm == 0))
        if n0 == 64 and np.all(fm == fm[0]):   # 64 equal values: every stage of the sum tree doubles
            s1, s2, exact = 64.0 * float(fm[0]), 64.0 * float(fm[0] * fm[0]), True
        m1 = s1 / n0
        scale = s2 / n0
        if not exact and np.abs(fm).max() < 1e-12 * max(np.abs(d).max(), 1e-300):
            return 0.0, np.inf     # the deviations themselves are fp64 rounding (collinear samples)
        return s2 / n0 - m1 * m1, (0.0 if exact else 1e-5 * scale + 1e-300)
    n0 = min(n, block)
    fa = (pts[:n0, 0] - pts[0, 0]).astype(f32)
    fb = (pts[:n0, 1] - pts[0, 1]).astype(f32)
    sa, sb = float(fa.sum(dtype=f32)), float(fb.sum(dtype=f32))
    saa, sbb = float((fa * fa).sum(dtype=f32)), float((fb * fb).sum(dtype=f32))
    sab = float((fa * fb).sum(dtype=f32))
    ma, mb = sa / n0, sb / n0
    cxx, cyy, cxy = saa / n0 - ma * ma, sbb / n0 - mb * mb, sab / n0 - ma * mb
    var = h[0] * h[0] * cxx + 2.0 * h[0] * h[1] * cxy + h[1] * h[1] * cyy
    exact = bool(np.all(fa == 0) and np.all(fb == 0)) or (h[1] == 0.0 and bool(np.all(fa == 0)))
    scale = h[0] * h[0] * saa / n0 + h[1] * h[1] * sbb / n0
    return var, (0.0 if exact else 1e-5 * scale + 1e-300)


def predict_path(pts, h, alpha, block, per, log_nb):
    """The one class of predict_paths, or UNSURE."""
    out = predict_paths(pts, h, alpha, block, per, log_nb)
    return next(iter(out)) if len(out) == 1 else UNSURE


def predict_paths(pts, h, alpha, block, per, log_nb):
    """Which way the kernel's selection goes for one unit (pts [N, 2] fp64, h the unit's fp64
    direction): FAST (target bucket inside the window, <= 128 candidates), BELOW / ABOVE (tau
    outside the window), CROWDED (> 128 candidates), NOVAR (window variance not positive), or
    {UNSURE} where the variance is not clear of its own fp32 rounding.  Returns the set of classes
    that come out with sd_d scaled by 0.9, 1.0 and 1.1: a prediction is robust when it has one
    element.  Certifies test inputs; never compared with the kernel."""
    n = len(pts)
    mu = pts.mean(axis=0)
    var, noise = window_variance(pts, h, mu, block, per)
    if noise == 0.0 and not var > 0.0:
        return {NOVAR}
    if not var > noise:
        return {UNSURE}
    z_lo, wsd, rank = window_params(alpha, n)
    nb = 1 << log_nb
    d = h[0] * pts[:, 0] + h[1] * pts[:, 1]
    mu_d = h[0] * mu[0] + h[1] * mu[1]
    out = set()
    for f in (0.9, 1.0, 1.1):
        sd = math.sqrt(var) * f
        tpos = (d - (mu_d + z_lo * sd)) * (nb / (2.0 * wsd) / sd)
        below = int((tpos < 0).sum())
        inside = tpos[(tpos >= 0) & (tpos < nb)].astype(np.int64)
        if rank < below:
            out.add(BELOW)
        elif rank - below >= len(inside):
            out.add(ABOVE)
        else:
            counts = np.bincount(inside, minlength=nb)
            b = int(np.searchsorted(np.cumsum(counts), rank - below, side="right"))
            out.add(CROWDED if counts[b] > K_CAP else FAST)
    return out
