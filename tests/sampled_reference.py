"""Helper of tests/test_sampled_host.py (CPU) and tests/test_sampled_halfspaces.py (GPU): the test
grid, the sizes and a window mirror of the sampled-halfspace kernel (csrc/drcvar_sampled.hip).
Plain NumPy, never the product path, and it does not import the engine.  The reference, its error
bound, the alpha classes and the rank mutations are those of tests/halfspace_reference.py.

Window mirror
-------------
The kernel places its histogram window from the KNOWN distribution of the projections:
``sd_d^2 = (l00 h0 + l10 h1)^2 + (l11 h1)^2`` about the unit's own ``mu_d``, with the stored
form's ``z_lo``, ``window_sd`` (``halfspace_reference.window_params``) and the plan's bin count.
``classify`` names the way a unit's selection goes:

* ``SETTLED``   the noise-free step 0: no window, tau = the nominal point's projection;
* ``FAST``      tau's bucket lies in the window and holds <= 128 samples;
* ``BELOW`` / ``ABOVE``   tau lies outside the window;
* ``CROWDED``   tau's bucket holds more than 128 samples;
* ``NOWINDOW``  sd_d is not positive or not finite (a zero or overflowing factor).

All but SETTLED and FAST enter the exact fallback (select_exact of csrc/drcvar_selection.inc, the
stored form's own routine) over the kernel's registers.  A class is reported
only when it is the same with sd_d scaled by 0.99, 1 and 1.01; otherwise ``UNSURE``.  The mirror
works in long double on the stored samples.  Where every sample of a noisy unit is the same point
(noise below one ulp of the position, sd_d > 0) it has d - mu_d = 0 exactly, and the class follows
from alpha alone: z_alpha within the window's half-width of 0 puts all N samples into one bucket
(CROWDED for N > 128), a lower alpha leaves them all above the window (ABOVE), a higher one all
below it (BELOW).  The kernel's own d - mu_d is there its rounding, a few ulp at most, which can
move the unit between these three entrances of the same fallback; the mirror certifies the inputs,
it is never compared with the kernel.

Which plan can reach which class: every plan reaches SETTLED and FAST.  CROWDED needs more than 128
samples in one bucket, so the 64 x 1 plan (N <= 128) cannot reach it; and at N <= 128 the window's
half-width (at least 12 standard errors of the sample quantile) exceeds |z_alpha| in every alpha
class, so a unit whose samples all sit at mu_d lies inside the window: that plan reaches neither
BELOW nor ABOVE.  Every other plan reaches all five at its full size.
"""
import math

import numpy as np

import halfspace_reference as hr

LD = np.longdouble
# (threads, Philox pairs per thread, log2 bins) of the kernel's launch plans: 2 * threads * pairs
# samples each, the smallest that holds N
PLANS = [(64, 1, 7), (256, 1, 8), (512, 1, 9), (512, 2, 10), (512, 4, 10), (512, 8, 10),
         (1024, 8, 10)]
MAX_SAMPLES = 16384
SETTLED, FAST, BELOW, ABOVE, CROWDED, NOWINDOW, UNSURE = (
    "SETTLED", "FAST", "BELOW", "ABOVE", "CROWDED", "NOWINDOW", "UNSURE")
CLASSES = (SETTLED, FAST, BELOW, ABOVE, CROWDED)

ISO, GENERAL = (0.1, 0.0, 0.1), (0.1, 0.05, 0.2)
WIDE_ISO, WIDE_GENERAL = (2.0, 0.0, 2.0), (2.0, 1.0, 4.0)    # N >= 8193 (see factors_of)
O, T = 3, 4


def capacity(plan):
    return 2 * plan[0] * plan[1]


def plan_of(n):
    for p in PLANS:
        if n <= capacity(p):
            return p
    return None


def sizes_of(plan):
    """The sizes a plan is tested at: full, one pair into its last row of pairs (or the plan's
    smallest size, where that is larger), an odd one (and the tiny ones on the smallest plan)."""
    i = PLANS.index(plan)
    lower = capacity(PLANS[i - 1]) if i else 0
    full = capacity(plan)
    s = [full, max(2 * (plan[0] * (plan[1] - 1) + 1), lower + 1), ((lower + full) // 2) | 1]
    if i == 0:
        s += [1, 2, 3, 63, 64, 65]
    return sorted(set(s))


def factors_of(n):
    """The two Cholesky factors (isotropic, general) a size is compared at.  From N = 8193 the
    noise is wider: the reference's bound there is dominated by the mean's summation term, and a
    rank off by one stays many bounds away only with more spread (tests/test_sampled_host.py)."""
    return (WIDE_ISO, WIDE_GENERAL) if n >= 8193 else (ISO, GENERAL)


def grid(seed=7):
    """(nominal [O, T, 2] uniform in [-5, 5]^2, ego [T, 2] a short line outside that square, the
    per-unit ego [O T, 2])."""
    rng = np.random.default_rng(seed)
    nominal = rng.uniform(-5.0, 5.0, size=(O, T, 2))
    ego = np.stack([-7.0 + 0.5 * np.arange(T), -6.0 + 0.25 * np.arange(T)], axis=1)
    return nominal, ego, np.ascontiguousarray(np.tile(ego, (O, 1)))


def noise_free_units(zero_first_step=True):
    return np.array([zero_first_step and (u % T == 0) for u in range(O * T)])


def sd_d(h, chol):
    l00, l10, l11 = chol
    s0, s1 = l00 * h[0] + l10 * h[1], l11 * h[1]
    with np.errstate(over="ignore"):
        return float(np.sqrt(np.float64(s0) * s0 + np.float64(s1) * s1))


def classify_set(pts, h, chol, alpha, log_nb, noise_free=False):
    """The classes of one unit (pts [N, 2] fp64, h its fp64 direction) with sd_d scaled by 0.99, 1
    and 1.01."""
    if noise_free:
        return {SETTLED}
    sd = sd_d(h, chol)
    if not (sd > 0.0 and math.isfinite(sd)):
        return {NOWINDOW}
    n = len(pts)
    z_lo, wsd, rank = hr.window_params(alpha, n)
    nb = 1 << log_nb
    p = np.asarray(pts, dtype=np.float64).astype(LD)
    p = p - p[0]          # about the first sample: a unit of equal samples has d - mu_d = 0 exactly
    mu = p.sum(axis=0) / LD(n)
    dev = (LD(h[0]) * p[:, 0] + LD(h[1]) * p[:, 1]) - (LD(h[0]) * mu[0] + LD(h[1]) * mu[1])
    out = set()
    for f in (0.99, 1.0, 1.01):
        with np.errstate(over="ignore", invalid="ignore"):
            tpos = (dev / LD(sd * f) - LD(z_lo)) * LD(nb / (2.0 * wsd))
        below = int((tpos < 0).sum())
        inside = np.floor(tpos[(tpos >= 0) & (tpos < nb)]).astype(np.int64)
        if rank < below:
            out.add(BELOW)
        elif rank - below >= len(inside):
            out.add(ABOVE)
        else:
            counts = np.bincount(inside, minlength=nb)
            b = int(np.searchsorted(np.cumsum(counts), rank - below, side="right"))
            out.add(CROWDED if counts[b] > hr.K_CAP else FAST)
    return out


def classify(pts, h, chol, alpha, log_nb, noise_free=False):
    s = classify_set(pts, h, chol, alpha, log_nb, noise_free)
    return next(iter(s)) if len(s) == 1 else UNSURE


def classify_units(samples, ref, chol, alpha, log_nb, zero_first_step=True):
    """One class per unit of a [O T, N, 2] draw (`ref` = halfspace_reference.reference of it)."""
    nf = noise_free_units(zero_first_step)
    return [classify(samples[i], ref.rec[i, 3:5], chol, alpha, log_nb, bool(nf[i]))
            for i in range(len(samples))]
