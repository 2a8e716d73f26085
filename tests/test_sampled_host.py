"""CPU: the host side of the sampled-halfspace entry (drcvar_sampled_halfspaces_f64,
csrc/drcvar_sampled.hip) — every validation exit, with no call reaching a device; the launch plans;
the window mirror of tests/sampled_reference.py on mirror-drawn units; and the check that the GPU
comparisons of tests/test_sampled_halfspaces.py can fail: on the same kind of draw, a rank off by
one lies outside the reference's bound."""
import ctypes
import functools

import numpy as np
import pytest

import halfspace_reference as hr
import sampled_reference as sr
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native
from oracle import philox_sampler as ps

SEED, STREAM = 11, 3


def _call(lib, **kw):
    a = dict(nominal=16, O=3, T=4, nso=8, nst=2, u0=0, count=12, N=100, l=(0.1, 0.0, 0.1), seed=1,
             stream_offset=0, zf=1, ego=16, es=2, rr=0.3, ro=0.3, alpha=0.2, delta=0.1, eps=0.15,
             out=16, status=None, samples=None, su=200, sn=2)
    a.update(kw)
    return lib.drcvar_sampled_halfspaces_f64(
        ctypes.c_void_p(a["nominal"]), a["O"], a["T"], a["nso"], a["nst"], a["u0"], a["count"],
        a["N"], *a["l"], a["seed"], a["stream_offset"], a["zf"], ctypes.c_void_p(a["ego"]),
        a["es"], a["rr"], a["ro"], a["alpha"], a["delta"], a["eps"], ctypes.c_void_p(a["out"]),
        ctypes.c_void_p(a["status"]), ctypes.c_void_p(a["samples"]), a["su"], a["sn"], None)


def test_host_side_argument_validation():
    """Every exit is taken before any launch: the pointers are not device memory."""
    lib = _native.lib()
    inv, uns, nan = _native.ERR_INVALID_ARGUMENT, _native.ERR_UNSUPPORTED, float("nan")
    for null in ("nominal", "ego", "out"):
        assert _call(lib, **{null: None}) == inv, null
    for neg in ("O", "T", "N", "u0", "count"):
        assert _call(lib, **{neg: -1}) == inv, neg
    # a unit range outside the grid
    assert _call(lib, u0=13, count=0) == inv
    assert _call(lib, u0=1, count=12) == inv
    assert _call(lib, u0=12, count=1) == inv
    assert _call(lib, T=0, count=1) == inv
    # NaN parameters (and the alpha the stored form rejects)
    for l in ((nan, 0.0, 0.1), (0.1, nan, 0.1), (0.1, 0.0, nan)):
        assert _call(lib, l=l) == inv
    for name in ("rr", "ro", "alpha", "delta", "eps"):
        assert _call(lib, **{name: nan}) == inv, name
    assert _call(lib, alpha=0.0) == inv and _call(lib, alpha=-0.2) == inv
    # beyond the register plans, beyond the sampler's grid
    assert _call(lib, N=_native.MAX_SAMPLES + 1) == uns
    assert _call(lib, O=(1 << 40) + 1, T=1) == uns
    assert _call(lib, O=1, T=(1 << 40) + 1) == uns
    assert _call(lib, O=1 << 21, T=1 << 21) == uns
    assert _call(lib, O=1 << 20, T=1 << 20, u0=0, count=1 << 31) == uns   # one workgroup per unit
    # nothing to do: no launch, the pointers are not looked at
    assert _call(lib, count=0) == _native.OK
    assert _call(lib, N=0) == _native.OK
    assert _call(lib, u0=12, count=0, nominal=None, ego=None, out=None) == _native.OK
    assert _call(lib, O=0, count=0) == _native.OK


def test_launch_plan_covers_every_size_at_the_boundaries():
    seen = []
    for plan in sr.PLANS:
        i = sr.PLANS.index(plan)
        lower = sr.capacity(sr.PLANS[i - 1]) if i else 0
        for n in {lower + 1, lower + 2, sr.capacity(plan) - 1, sr.capacity(plan)} | set(sr.sizes_of(plan)):
            threads, pairs = _native.sampled_launch_plan(n)
            assert (threads, pairs) == plan[:2], n
            assert 2 * threads * pairs >= n and threads % 64 == 0 and threads <= 1024
            assert sr.plan_of(n) == plan
        seen.append(plan[:2])
    assert len(set(seen)) == len(sr.PLANS) and sr.capacity(sr.PLANS[-1]) == _native.MAX_SAMPLES
    lib = _native.lib()
    assert lib.drcvar_sampled_launch_plan(100, None, None) == _native.OK
    for n, code in ((0, _native.ERR_INVALID_ARGUMENT), (-5, _native.ERR_INVALID_ARGUMENT),
                    (_native.MAX_SAMPLES + 1, _native.ERR_UNSUPPORTED)):
        with pytest.raises(_native.EngineError) as e:
            _native.sampled_launch_plan(n)
        assert e.value.code == code


def test_python_surface_rejects_before_the_device():
    import torch
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import engine
    nominal = torch.zeros((3, 4, 2), dtype=torch.float64)
    with pytest.raises(ValueError):
        engine.sampled_halfspaces(nominal, torch.zeros((4, 2), dtype=torch.float64), 100)


@functools.lru_cache(maxsize=None)
def _draw(n, chol):
    """The mirror's draw of the test grid, flat [O T, N, 2]."""
    nominal, _, _ = sr.grid()
    return ps.sample_trajectories(nominal, n, chol, SEED, STREAM).reshape(sr.O * sr.T, n, 2)


@pytest.mark.parametrize("n", [2, 3, 63, 129, 1000, 5001, 8193, 16384])
def test_a_rank_off_by_one_lies_outside_the_bound(n):
    """On the mirror's draws of the test grid, g_cvar with tau taken one rank too low or too high
    (a consistent tail sum) lies outside Ref.bound for every noisy unit, and for at least 80 % of
    the applicable (unit, mutant) pairs by four bounds or more — in every (factor, alpha class)
    case.  A condition on the inputs: where it fails the noise is widened, never the bound.  The
    noise-free units are exempt (a rank shift inside a tie is a no-op)."""
    _, _, ego_u = sr.grid()
    noisy = ~sr.noise_free_units()
    assert _native.sampled_launch_plan(n) == sr.plan_of(n)[:2]   # a size the kernel runs, on this plan
    for chol in sr.factors_of(n):
        s = _draw(n, chol)
        for a0 in hr.A0:
            alpha, _ = hr.alpha_of(n, a0)
            ref = hr.reference(s, ego=ego_u, alpha=alpha)
            dist = []
            for i in np.flatnonzero(noisy):
                for kind in ("rank_lo", "rank_hi"):
                    g = hr.mutated_g_cvar(ref, i, kind)
                    if g is not None:
                        dist.append(abs(g - ref.rec[i, 5]) / ref.bound[i])
            assert dist, (n, chol, a0)
            dist = np.array(dist)
            print(f"N={n} chol={chol} a0={a0}: {len(dist)} pairs, min {dist.min():.3g} bounds, "
                  f"{(dist >= 4).mean():.0%} sharp")
            assert dist.min() > 1.0, (n, chol, a0, dist.min())
            assert (dist >= 4.0).mean() >= 0.8, (n, chol, a0, np.sort(dist)[:6])


def test_window_mirror_on_mirror_drawn_units():
    """The classifier on the mirror's draws: noise-free units SETTLED; Gaussian units FAST in every
    alpha class (the window is placed from the true distribution, at least 12 standard errors of
    the sample quantile either side); a zero factor has no window; noise below one ulp of the
    position leaves all samples one point with sd_d > 0, and the class follows from alpha:
    ABOVE, CROWDED (N > 128; FAST at N <= 128), BELOW."""
    nominal, _, ego_u = sr.grid()
    nf = sr.noise_free_units()
    for n in (65, 1000, 5001):
        plan = sr.plan_of(n)
        assert _native.sampled_launch_plan(n) == plan[:2]   # the mirror's bin count is this plan's
        for chol in (sr.ISO, sr.GENERAL):
            s = _draw(n, chol)
            for a0 in hr.A0:
                alpha, _ = hr.alpha_of(n, a0)
                ref = hr.reference(s, ego=ego_u, alpha=alpha)
                cls = sr.classify_units(s, ref, chol, alpha, plan[2])
                assert all(c == (sr.SETTLED if nf[i] else sr.FAST) for i, c in enumerate(cls)), (n, chol, a0, cls)
        flat = np.repeat(nominal.reshape(-1, 1, 2), n, axis=1)
        for a0 in hr.A0:
            alpha, _ = hr.alpha_of(n, a0)
            # all samples at mu_d: where 0 lies against the window [z_lo, z_lo + 2 window_sd) sd_d
            z_lo, wsd, _ = hr.window_params(alpha, n)
            want = (sr.BELOW if z_lo > 0 else sr.ABOVE if z_lo + 2 * wsd <= 0
                    else sr.CROWDED if n > hr.K_CAP else sr.FAST)
            if n == 5001:   # the window there is narrower than |z_alpha| away from the median
                assert want == {0.02: sr.ABOVE, 0.2: sr.ABOVE, 0.5: sr.CROWDED, 0.9: sr.BELOW}.get(a0, want)
            ref = hr.reference(flat, ego=ego_u, alpha=alpha)
            cls = sr.classify_units(flat, ref, (1e-20, 0.0, 1e-20), alpha, plan[2], zero_first_step=False)
            assert cls == [want] * len(cls), (n, a0, cls)
            assert sr.classify_units(flat, ref, (0.0, 0.0, 0.0), alpha, plan[2],
                                     zero_first_step=False) == [sr.NOWINDOW] * len(cls)
    # a unit whose class changes with sd_d within one per cent is not reported
    pts = np.stack([np.linspace(-1.0, 1.0, 200), np.zeros(200)], axis=1)
    edge = sr.classify_set(pts, (1.0, 0.0), (1.0, 0.0, 1.0), 0.999, 7)
    assert sr.classify(pts, (1.0, 0.0), (1.0, 0.0, 1.0), 0.999, 7) in (*sr.CLASSES, sr.UNSURE)
    assert (len(edge) == 1) == (sr.classify(pts, (1.0, 0.0), (1.0, 0.0, 1.0), 0.999, 7) != sr.UNSURE)
