"""NumPy mirror of the device Monte Carlo clearance kernel (csrc/drcvar_clearance.hip), built on the
sampler's mirror oracle/philox_sampler.py (philox4x32_10, log_u32, cos_sin_u32).  A helper of
tests/test_monte_carlo*.py, never the product path.

One Philox4x32-10 call per (m, o, t): counter (g lo, g hi, stream lo, stream hi) with
g = m (O T) + o T + t, key = seed.  Laplace: n = (bx (E(x0) - E(x1)), by (E(x2) - E(x3))),
E(x) = -log u32(x).  Gaussian: (x0, x1) -> Box-Muller -> z, n = L z.

Non-finite positions: ndarray.min propagates NaN, and that IEEE result is the kernel's contract
(include/drcvar_sampling.h): a NaN d^2 makes its clearance NaN and its step count nothing.
"""
import numpy as np

from oracle import philox_sampler as ps

_MASK32 = np.uint64(0xFFFFFFFF)


def noise(kind, params, O, T, M, seed, stream_offset=0, first_realization=0, zero_first_step=True):
    """[M, O, T, 2] noise of realisations first_realization .. first_realization + M - 1.
    kind "laplace": params (bx, by); "gaussian": params (l00, l10, l11)."""
    m = np.arange(first_realization, first_realization + M, dtype=np.uint64).reshape(M, 1, 1)
    o = np.arange(O, dtype=np.uint64).reshape(1, O, 1)
    t = np.arange(T, dtype=np.uint64).reshape(1, 1, T)
    g = (m * np.uint64(O * T) + o * np.uint64(T) + t).reshape(-1)
    x0, x1, x2, x3 = ps.philox4x32_10(g & _MASK32, g >> np.uint64(32),
                                      np.uint64(stream_offset & 0xFFFFFFFF),
                                      np.uint64((stream_offset >> 32) & 0xFFFFFFFF),
                                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = np.empty((M * O * T, 2))
    if kind == "laplace":
        bx, by = params
        out[:, 0] = bx * ((-ps.log_u32(x0)) - (-ps.log_u32(x1)))
        out[:, 1] = by * ((-ps.log_u32(x2)) - (-ps.log_u32(x3)))
    elif kind == "gaussian":
        l00, l10, l11 = params
        rad = np.sqrt(-2.0 * ps.log_u32(x0))
        cs, sn = ps.cos_sin_u32(x1)
        z0, z1 = rad * cs, rad * sn
        out[:, 0] = l00 * z0
        out[:, 1] = l10 * z0 + l11 * z1
    else:
        raise ValueError(kind)
    out = out.reshape(M, O, T, 2)
    if zero_first_step and T:
        out[:, :, 0] = 0.0
    return out


def step_min_d2(ego, nominal, noise_motk):
    """[K, M, T]: min over o of |ego[k, t] - (nominal[o, t] + noise[m, o, t])|^2."""
    pos = np.asarray(nominal)[None] + noise_motk                         # [M, O, T, 2]
    d = np.asarray(ego)[:, None, None] - pos[None]                       # [K, M, O, T, 2]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).min(axis=2)


def min_clearance(ego, nominal, noise_motk, combined_radius):
    """(min_clearance [K, M], step_hits [K, T], margin): sqrt(min d^2) - R, the per-step collision
    counts #{m : min_o d^2 < R R}, and the smallest |min_o d^2 - R R| (how far the hit counts are
    from depending on rounding)."""
    d2 = step_min_d2(ego, nominal, noise_motk)
    rr = combined_radius * combined_radius
    clr = np.sqrt(d2.min(axis=2)) - combined_radius
    hits = (d2 < rr).sum(axis=1).astype(np.int64)
    margin = float(np.min(np.abs(d2 - rr))) if d2.size else np.inf
    return clr, hits, margin
