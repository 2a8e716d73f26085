"""GPU: the finish of the fused halfspace kernel after the histogram scan — the one-trip layout of
small target buckets (c <= 64 / NW: all candidates in cand[0 .. 64), `rank_candidates_express`)
against the per-wave regions of larger ones.

One launch per geometry through `drcvar_offsets_given_h_f64_v2` with h = [1, 0], so that d = x
exactly and the planted values are the projections themselves.  Every unit is a seeded Gaussian
spread whose values around rank m = floor(alpha N) are replaced by a cluster of c planted values
inside a span of 1e-6 sd (a bin of the window is 2e-3 sd or wider), with a gap of several bins on
both sides, so that the target bucket holds exactly the cluster:

* c in {1, 2, NW, 64/NW - 1, 64/NW, 64/NW + 1, 64, 65, 128} as far as N allows — both sides of
  the threshold between the two layouts and of the one- / two-register ranking (64 | 65);
* the cluster placed by sample index: all in wave 0, all in the last wave, one per wave in turn,
  in the (partly filled) last row;
* distinct values, two equal values with tau among them, c equal values;
* rank m the first, the middle and the last of the cluster.

`bucket_count` restates the kernel's window from tests/halfspace_reference.py (window_variance,
window_params) on the CPU and certifies each unit's class before anything runs on the device: a
cluster that straddles a bin edge is re-seeded, an uncertified unit or an empty class fails.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import halfspace_reference as hr

pytestmark = pytest.mark.gpu

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams  # noqa: E402

DEV = torch.device("cuda", 0)
SIGMA = hr.SIGMA
SPAN = 1e-6 * SIGMA          # width of the planted cluster
GAP_BINS = 8                 # clear space on both sides of it, in nominal bins of the window
A0_CLASS = 3                 # hr.A0[3] = 0.5: the cluster sits at the median, inside any window
PLACEMENTS = ("wave0", "last_wave", "round_robin", "last_row")
RANKPOS = ("first", "middle", "last")
TIES = ("distinct", "two_equal", "all_equal")

# (threads, per thread, log2 bins), N of the given-h launch (the automatic chain picks the
# geometry), and another compiled geometry covering N for the `_ex` launch: 512 x 2 (NW = 8:
# segments of 8 candidates), 128 x 8 (NW = 2), 64 x 16 (one wave, tail partials reduced per wave)
CASES = [((256, 4, 9), 1000, (512, 2)), ((256, 4, 9), 1024, (512, 2)),
         ((128, 4, 8), 300, (128, 8)), ((64, 2, 7), 100, (64, 16))]
IDS = [f"{g[0]}x{g[1]}-N{n}" for g, n, _ in CASES]


def cluster_sizes(nw):
    e = 64 // nw
    return sorted({1, 2, nw, e - 1, e, e + 1, 64, 65, 128})


def size_class(c, nw):
    """0: c = 1; 1: 2 .. 64/NW (one-trip layout); 2: 64/NW + 1 .. 64; 3: 65 .. 128."""
    return 0 if c == 1 else 1 if c <= 64 // nw else 2 if c <= 64 else 3


def bucket_count(pts, alpha, block, per, log_nb):
    """The number of samples in the target bucket of the kernel's first-pass window for one unit
    with h = [1, 0], or None where the selection does not end in that bucket or the count depends
    on the last digits of the window's fp32 variance (sd scaled by 1 -+ 1e-3: a thousand times
    the rounding of its sums) — a cluster on a bin edge."""
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


def _slots(placement, n, block, per):
    """Sample indices a placement may use, as one list per wave taken in turn."""
    nw = block // 64
    i = np.arange(n)
    wave = (i % block) // 64
    if placement == "wave0":
        return [i[wave == 0]]
    if placement == "last_wave":
        return [i[wave == nw - 1]]
    if placement == "round_robin":
        return [i[wave == w] for w in range(nw)]
    return [i[i >= ((n - 1) // block) * block]]        # last_row


def make_unit(c, placement, rankpos, tie, n, m, geometry, alpha, seed):
    """pts [n, 2] of one unit, or None where the combination does not fit n (rank window past
    either end, fewer slots than c)."""
    block, per, log_nb = geometry
    p = {"first": 0, "middle": c // 2, "last": c - 1}[rankpos]
    lo = m - p
    if lo < 0 or lo + c > n:
        return None
    rng = np.random.default_rng([n, c, PLACEMENTS.index(placement), RANKPOS.index(rankpos),
                                 TIES.index(tie), seed])
    pools = [rng.permutation(s) for s in _slots(placement, n, block, per)]
    if -(-c // len(pools)) > min(len(s) for s in pools):
        return None
    idx = np.array([pools[k % len(pools)][k // len(pools)] for k in range(c)])
    v = np.sort(rng.normal(size=n)) * SIGMA + rng.uniform(-3, 3)
    centre = v[m]
    cv = centre + SPAN * (np.arange(c) / max(c - 1, 1) - 0.5)     # sorted, distinct
    if tie == "two_equal" and c >= 2:
        cv[p + 1 if p + 1 < c else p - 1] = cv[p]
    elif tie == "all_equal":
        cv[:] = centre
    _, wsd, _ = hr.window_params(alpha, n)
    gap = GAP_BINS * 2.0 * wsd * SIGMA / (1 << log_nb)
    others = np.concatenate([v[:lo] - gap, v[lo + c:] + gap])
    x = np.empty(n)
    rest = np.ones(n, dtype=bool)
    rest[idx] = False
    x[idx] = rng.permutation(cv)
    x[rest] = rng.permutation(others)
    return np.stack([x, rng.normal(size=n) * SIGMA + rng.uniform(-3, 3)], axis=1)


@functools.lru_cache(maxsize=None)
def batch(case):
    """The certified units of one geometry: dict(samples [U, N, 2], c [U], labels, alpha, m)."""
    geometry, n, _ = CASES[case]
    block, per, log_nb = geometry
    nw = block // 64
    alpha, m = hr.alpha_of(n, hr.A0[A0_CLASS])
    units, cs, labels = [], [], []
    k = 0
    for c in cluster_sizes(nw):
        for placement in PLACEMENTS:
            k += 1
            # rank position and ties walk with the unit's number; a combination that does not fit
            # N moves on to the next one, so that a (c, placement) is dropped only when none fits
            for step in range(len(RANKPOS) * len(TIES)):
                rankpos = RANKPOS[(k + step) % 3]
                tie = TIES[((k + step) // 3) % 3] if c > 1 else "distinct"
                label = f"c{c}-{placement}-{rankpos}-{tie}"
                if make_unit(c, placement, rankpos, tie, n, m, geometry, alpha, 0) is None:
                    continue
                for seed in range(32):      # a cluster on a bin edge: another seed
                    pts = make_unit(c, placement, rankpos, tie, n, m, geometry, alpha, seed)
                    if bucket_count(pts, alpha, block, per, log_nb) == c:
                        break
                else:
                    raise AssertionError(f"{IDS[case]} {label}: no seed puts {c} in the bucket")
                units.append(pts)
                cs.append(c)
                labels.append(label)
                break
    samples = np.ascontiguousarray(np.stack(units))
    return dict(samples=samples, c=np.array(cs), labels=labels, alpha=alpha, m=m)


@functools.lru_cache(maxsize=None)
def ref_given(case):
    b = batch(case)
    h = np.tile([1.0, 0.0], (len(b["samples"]), 1))
    return hr.reference(b["samples"], h=h, alpha=b["alpha"])


def _params(alpha):
    return RiskParams(hr.RR, hr.RO, alpha, hr.DELTA, hr.EPSILON)


def _launch_given(b):
    s = torch.as_tensor(b["samples"]).to(DEV)
    h = torch.tensor([[1.0, 0.0]], dtype=torch.float64).repeat(s.shape[0], 1).to(DEV)
    status = torch.full((s.shape[0],), -1, dtype=torch.int32, device=DEV)
    out = engine.offsets_given_h(s, h, _params(b["alpha"]), status=status)
    torch.cuda.synchronize()
    return out, status


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_buckets_hold_the_planted_clusters(case):
    """Every unit's target bucket holds its c (host restatement of the window), no unit is left
    out, and every size class the geometry can hold has a unit."""
    geometry, n, _ = CASES[case]
    block, per, log_nb = geometry
    nw = block // 64
    b = batch(case)
    assert len(b["labels"]) >= 12
    for pts, c, label in zip(b["samples"], b["c"], b["labels"]):
        assert bucket_count(pts, b["alpha"], block, per, log_nb) == c, label
        d = np.sort(pts[:, 0])
        assert (np.abs(d - d[b["m"]]) <= 1.5 * SPAN).sum() == c, label   # tau is of the cluster
    have = {size_class(int(c), nw) for c in b["c"]}
    want = {0, 1, 2, 3} if nw > 1 else {0, 1, 3}     # (one wave: 64 / NW = 64, no class 2)
    assert have >= want, (IDS[case], have)
    for placement in PLACEMENTS:
        assert any(f"-{placement}-" in lb for lb in b["labels"])
    for word in RANKPOS + TIES:
        assert any(f"-{word}" in lb for lb in b["labels"]), word


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_offsets_at_the_bound(case):
    """Columns 5..7 within the reference's derived per-unit bound, columns 0..4 at 1e-12, status
    0; a second launch gives the same bits."""
    b, ref = batch(case), ref_given(case)
    out, status = _launch_given(b)
    got = out.cpu().numpy()
    assert (status.cpu().numpy() == _native.UNIT_OK).all()
    assert ref.ok.all()
    err = np.abs(got - ref.rec)
    ratio = err[:, 5:8] / ref.bound[:, None]
    print(f"RATIO {IDS[case]} max error / bound {ratio.max():.3f}")
    bad = np.argwhere(ratio > 1.0)
    assert bad.size == 0, [(b["labels"][i], int(j) + 5, got[i, j + 5], ref.rec[i, j + 5],
                            ref.bound[i]) for i, j in bad[:6]]
    assert (err[:, 0:5] <= 1e-12).all(), [b["labels"][i] for i in np.argwhere(err[:, 0:5] > 1e-12)[:6, 0]]
    out2, status2 = _launch_given(b)
    assert torch.equal(out, out2) and torch.equal(status, status2)


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_other_geometry_agrees(case):
    """The same batch with ego = mean - 3 [1, 0] (h = [1, 0] up to rounding) through
    drcvar_safe_halfspaces_f64_ex on another geometry covering N: within the reference's bounds."""
    _, n, other = CASES[case]
    b = batch(case)
    ego = b["samples"].mean(axis=1) - hr.RHO * np.array([1.0, 0.0])
    ref = hr.reference(b["samples"], ego=ego, alpha=b["alpha"])
    s = torch.as_tensor(b["samples"][None]).to(DEV)            # [1, U, N, 2]: the units along T
    e = torch.as_tensor(np.ascontiguousarray(ego)).to(DEV)
    out = torch.empty((1, s.shape[1], _native.OUT_WIDTH), dtype=torch.float64, device=DEV)
    p = _params(b["alpha"])
    _native.check(_native.lib().drcvar_safe_halfspaces_f64_ex(
        ctypes.c_void_p(s.data_ptr()), 1, s.shape[1], n, s.stride(0), s.stride(1), s.stride(2),
        ctypes.c_void_p(e.data_ptr()), e.stride(0), p.robot_radius, p.obstacle_radius, p.alpha,
        p.delta, p.epsilon, ctypes.c_void_p(out.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream), other[0], other[1]))
    torch.cuda.synchronize()
    got = out[0].cpu().numpy()
    assert ref.ok.all()
    tol = np.stack([ref.bound_hm, ref.bound_hm, ref.bound_gm, ref.bound_h, ref.bound_h,
                    ref.bound, ref.bound, ref.bound], axis=1)
    err = np.abs(got - ref.rec)
    print(f"RATIO {IDS[case]} on {other} max error / bound {(err[:, 5:8] / tol[:, 5:8]).max():.3f}")
    bad = np.argwhere(err > tol)
    assert bad.size == 0, [(b["labels"][i], int(j), got[i, j], ref.rec[i, j], tol[i, j])
                           for i, j in bad[:6]]
