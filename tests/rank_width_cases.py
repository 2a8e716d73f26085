"""Planted target buckets for tests/test_halfspace_rank_width.py: plain NumPy on top of
tests/halfspace_reference.py, never the product path, and it does not import the engine.

Every unit is a seeded Gaussian spread along x (sd SIGMA) whose values around rank m = floor(N / 2)
are replaced by a cluster of c planted values SPACING apart, with GAP_BINS bins of the window
cleared on both sides, so that the kernel's target bucket holds exactly the cluster.  The direction
is [1, 0] (given, or from ego = mean - RHO [1, 0]), so the projections are the x themselves up to
the rounding of the direction.

What varies per plan (threads x samples per thread; E = 64 / waves):

* c in {1, 2, 3, 4, 5, 6, 8, E, E + 1}: the express ranking's straight-line visit alone, one to
  several trips of its loop (both sides of a block of four visits, the width a flat-cost form of
  the ranking was tried at), a full segment, and the first bucket that leaves the express path;
* the wanted rank first, second, last but one and last among the candidates;
* ties: distinct values; tau twice; tau four times; all c equal (tied samples share y as well, so
  that they stay tied under any direction);
* placement by sample index modulo the workgroup size: all candidates in one wave's samples, or
  one per wave in turn.

SPACING is chosen so that tau taken one rank too low or too high moves g_cvar by at least 30 of
the reference's bounds wherever the neighbour is not tied with tau: L moves by (k - m) SPACING / k
= SPACING / N at alpha = (m + 0.5) / N, i.e. 5e-10 at N = 2000, against bounds of about 1e-12 (the
ego form at N = 2000, where the direction's own bound dominates) and less elsewhere.
`bucket_count` restates the kernel's window and bin map and counts the target bucket on the CPU.
"""
import functools
import math

import numpy as np

import halfspace_reference as hr

SIGMA = hr.SIGMA
SPACING = 1e-6               # between neighbours of the planted cluster
GAP_BINS = 8                 # clear space on both sides of it, in bins of the window
MIN_GAP_BOUNDS = 30.0        # a rank off by one moves g_cvar by at least this many bounds
# (threads, samples per thread, log2 bins) and the N the automatic chain runs on it
PLANS = [((64, 2, 7), 128), ((128, 4, 8), 512), ((256, 4, 9), 1000), ((256, 8, 10), 2000)]
IDS = [f"{g[0]}x{g[1]}-N{n}" for g, n in PLANS]
RANKPOS = ("first", "second", "last_but_one", "last")
TIES = ("distinct", "tau_twice", "tau_four_times", "all_equal")
PLACEMENTS = ("one_wave", "one_per_wave")


def bucket_sizes(block):
    e = 64 // (block // 64)
    return sorted({1, 2, 3, 4, 5, 6, 8, e, e + 1})


def bucket_count(pts, alpha, block, per, log_nb):
    """Samples in the target bucket of the kernel's first-pass window for one unit with
    h = [1, 0], or None where the selection does not end in that bucket or the count changes with
    the window's sd scaled by 1 -+ 1e-3 (a thousand times the rounding of its fp32 sums): a
    cluster on a bin edge."""
    h = np.array([1.0, 0.0])
    n = len(pts)
    mu = pts.mean(axis=0)
    var, noise = hr.window_variance(pts, h, mu, block, per)
    if not var > max(noise, 0.0):
        return None
    z_lo, wsd, rank = hr.window_params(alpha, n)
    nb = 1 << log_nb
    d = pts[:, 0]
    found = set()
    for f in (0.999, 1.0, 1.001):
        sd = math.sqrt(var) * f
        tpos = (d - (mu[0] + z_lo * sd)) * (nb / (2.0 * wsd) / sd)
        below = int((tpos < 0).sum())
        inside = tpos[(tpos >= 0) & (tpos < nb)].astype(np.int64)
        if rank < below or rank - below >= len(inside):
            return None
        counts = np.bincount(inside, minlength=nb)
        b = int(np.searchsorted(np.cumsum(counts), rank - below, side="right"))
        found.add(int(counts[b]))
    return found.pop() if len(found) == 1 else None


def _position(rankpos, c):
    return {"first": 0, "second": 1, "last_but_one": c - 2, "last": c - 1}[rankpos]


def _tied(tie, c, p):
    """Indices of the sorted cluster that share tau's value (p among them), or None where the
    bucket is too small for the tie."""
    if tie == "distinct":
        return [p]
    if tie == "all_equal":
        return list(range(c)) if c >= 2 else None
    want = 2 if tie == "tau_twice" else 4
    if c < want:
        return None
    lo = min(max(p - want // 2 + 1, 0), c - want)
    return list(range(lo, lo + want))


def make_unit(c, rankpos, tie, placement, n, m, geometry, alpha, seed):
    """pts [n, 2] of one unit, or None where the combination does not exist (position outside the
    bucket, bucket too small for the tie, fewer slots than candidates)."""
    block, per, log_nb = geometry
    nw = block // 64
    p = _position(rankpos, c)
    if p < 0 or p >= c:
        return None
    tied = _tied(tie, c, p)
    if tied is None:
        return None
    lo = m - p
    if lo < 0 or lo + c > n:
        return None
    rng = np.random.default_rng([n, c, RANKPOS.index(rankpos), TIES.index(tie),
                                 PLACEMENTS.index(placement), seed])
    i = np.arange(n)
    wave = (i % block) // 64
    if placement == "one_wave":
        w = int(rng.integers(nw))
        pools = [rng.permutation(i[wave == w])]
    else:
        pools = [rng.permutation(i[wave == w]) for w in range(nw)]
    if -(-c // len(pools)) > min(len(s) for s in pools):
        return None
    idx = np.array([pools[k % len(pools)][k // len(pools)] for k in range(c)])
    v = np.sort(rng.normal(size=n)) * SIGMA + rng.uniform(-3, 3)
    cv = v[m] + SPACING * (np.arange(c) - p)          # sorted, distinct, cv[p] = the wanted rank's
    cv[tied] = cv[p]
    _, wsd, _ = hr.window_params(alpha, n)
    gap = GAP_BINS * 2.0 * wsd * SIGMA / (1 << log_nb) + SPACING * c
    others = np.concatenate([v[:lo] - gap, v[lo + c:] + gap])
    x = np.empty(n)
    y = rng.normal(size=n) * SIGMA + rng.uniform(-3, 3)
    rest = np.ones(n, dtype=bool)
    rest[idx] = False
    order = rng.permutation(c)
    x[idx] = cv[order]
    x[rest] = rng.permutation(others)
    if len(tied) > 1:                                  # tied under any direction
        y[idx[np.isin(order, tied)]] = y[idx[0]]
    return np.stack([x, y], axis=1)


@functools.lru_cache(maxsize=None)
def batch(plan):
    """The certified units of one plan: dict(samples [U, N, 2], c [U], labels, alpha, m)."""
    geometry, n = PLANS[plan]
    block, per, log_nb = geometry
    alpha, m = hr.alpha_of(n, 0.5)
    units, cs, labels = [], [], []
    k = 0
    for c in bucket_sizes(block):
        for rankpos in RANKPOS:
            if _position(rankpos, c) in [_position(r, c) for r in RANKPOS[:RANKPOS.index(rankpos)]]:
                continue                                # (c <= 3: positions coincide)
            for tie in TIES:
                k += 1
                # the placement alternates with the unit's number; one that does not fit the plan
                # (a wave with fewer slots than candidates) gives way to the other
                for placement in (PLACEMENTS[k % 2], PLACEMENTS[(k + 1) % 2]):
                    if make_unit(c, rankpos, tie, placement, n, m, geometry, alpha, 0) is None:
                        continue
                    label = f"c{c}-{rankpos}-{tie}-{placement}"
                    for seed in range(64):              # a cluster on a bin edge: another seed
                        pts = make_unit(c, rankpos, tie, placement, n, m, geometry, alpha, seed)
                        if bucket_count(pts, alpha, block, per, log_nb) == c:
                            break
                    else:
                        raise AssertionError(f"{IDS[plan]} {label}: no seed puts {c} in the bucket")
                    units.append(pts)
                    cs.append(c)
                    labels.append(label)
                    break
    return dict(samples=np.ascontiguousarray(np.stack(units)), c=np.array(cs), labels=labels,
                alpha=alpha, m=m)


def ego_of(samples):
    """One ego per unit, RHO behind the mean along x: the kernel's direction is [1, 0] up to the
    rounding of the mean."""
    return np.ascontiguousarray(samples.mean(axis=1) - hr.RHO * np.array([1.0, 0.0]))


@functools.lru_cache(maxsize=None)
def reference(plan, form):
    b = batch(plan)
    if form == "given_h":
        return hr.reference(b["samples"], h=np.tile([1.0, 0.0], (len(b["samples"]), 1)),
                            alpha=b["alpha"])
    return hr.reference(b["samples"], ego=ego_of(b["samples"]), alpha=b["alpha"])
