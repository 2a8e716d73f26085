"""GPU: the small plans' form without the `i < n` selects on the rows known full (the host picks it
when N > threads * (per - 1)), against the predicated form every other N runs.

For every automatic small plan, N on both sides of threads * (per - 1) and at the plan's end; one
launch of 10 units per N: 2 obstacles x 4 steps of seeded Gaussians, one unit whose samples are all
equal and one unit with a NaN sample (in row 0, a row whose selects the full-row form drops).  Each
launch runs through the ego form and the given-h form, from a 16-B-aligned buffer and from a view
8 bytes past 16-B alignment (the 8-B load form), and one explicit 256 x 4 launch at N = 100 leaves
three whole rows empty, so the host has to choose the predicated form for it.  Records and status
words are compared with the long-double reference of tests/halfspace_reference.py at its derived
per-unit bound; NaN and sentinel positions exactly; the 8-B form bit for bit with the 16-B form.
"""
import functools

import numpy as np
import pytest
import torch

import halfspace_reference as hr

pytestmark = pytest.mark.gpu

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams  # noqa: E402

DEV = torch.device("cuda", 0)
O, T = 2, 5                      # steps 0..3: Gaussians; step 4: the all-equal unit, the NaN unit
EQUAL, NAN_UNIT = 0 * T + 4, 1 * T + 4
NAN_INDEX = 5                    # row 0 of every plan
A0 = 0.2

# (threads, per thread, log2 bins) -> N: threads * (per - 1), one more, (C3's 1000,) the plan's end
PLANS = {(64, 2, 7): (64, 65, 128), (128, 4, 8): (384, 385, 512),
         (256, 4, 9): (768, 769, 1000, 1024), (256, 8, 10): (1792, 1793, 2048)}
CASES = [(plan, n) for plan, sizes in PLANS.items() for n in sizes]
IDS = [f"{p[0]}x{p[1]}-N{n}" for p, n in CASES]


@functools.lru_cache(maxsize=None)
def batch(n):
    """samples [O, T, n, 2], ego [T, 2], h [O * T, 2] (unit vectors), alpha."""
    rng = np.random.default_rng([n, 9])
    centre = rng.uniform(-4.0, 4.0, size=(O, T, 1, 2))
    s = centre + hr.SIGMA * rng.normal(size=(O, T, n, 2))
    s[0, 4] = s[0, 4, 0]                         # every sample of the unit equal
    s[1, 4, NAN_INDEX % n, 0] = np.nan
    ego = rng.uniform(-0.5, 0.5, size=(T, 2)) + np.array([6.0, 0.0])   # |mean - ego| >= 1.5
    ang = rng.uniform(0.0, 2.0 * np.pi, size=O * T)
    h = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    alpha, _ = hr.alpha_of(n, A0)
    return np.ascontiguousarray(s), ego, h, alpha


@functools.lru_cache(maxsize=None)
def ref_ego(n):
    s, ego, _, alpha = batch(n)
    return hr.reference(s.reshape(O * T, n, 2), ego=np.tile(ego, (O, 1)), alpha=alpha)


@functools.lru_cache(maxsize=None)
def ref_given(n):
    s, _, h, alpha = batch(n)
    return hr.reference(s.reshape(O * T, n, 2), h=h, alpha=alpha)


def _params(alpha):
    return RiskParams(hr.RR, hr.RO, alpha, hr.DELTA, hr.EPSILON)


def _device(a, unaligned):
    """`a` on the device; unaligned: its base 8 bytes past 16-byte alignment (the 8-B load form)."""
    t = torch.as_tensor(np.ascontiguousarray(a))
    if not unaligned:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=torch.float64, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8
    return v


def _run_ego(n, unaligned, geometry=None):
    s, ego, _, alpha = batch(n)
    status = torch.full((O * T,), -1, dtype=torch.int32, device=DEV)
    launch, out = engine.prepare_safe_halfspaces(_device(s, unaligned), _device(ego, False),
                                                 _params(alpha), geometry=geometry, status=status)
    launch()
    torch.cuda.synchronize()
    return out.reshape(O * T, _native.OUT_WIDTH), status


def _run_given(n, unaligned):
    s, _, h, alpha = batch(n)
    status = torch.full((O * T,), -1, dtype=torch.int32, device=DEV)
    out = engine.offsets_given_h(_device(s.reshape(O * T, n, 2), unaligned), _device(h, False),
                                 _params(alpha), status=status)
    torch.cuda.synchronize()
    return out, status


def _check(got, status, ref, label):
    """Records [U, 8] at the units' bounds; NaN and sentinel positions exact; the NaN unit holds the
    failure record (100, 100, 100 - R_c |h|) and the non-finite status word, every other unit 0."""
    got, status = got.cpu().numpy(), status.cpu().numpy()
    want = ref.rec
    assert not ref.ok[NAN_UNIT] and ref.ok.sum() == O * T - 1
    expect = np.zeros(O * T, dtype=np.int32)
    expect[NAN_UNIT] = _native.UNIT_NONFINITE
    np.testing.assert_array_equal(status, expect, err_msg=label)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=label)
    for c in (5, 6):
        np.testing.assert_array_equal(got[:, c] == hr.SENTINEL, want[:, c] == hr.SENTINEL, err_msg=label)
    assert got[NAN_UNIT, 5] == hr.SENTINEL and got[NAN_UNIT, 6] == hr.SENTINEL, label
    off = np.where(ref.ok, np.nan_to_num(ref.bound), 4 * hr.U64 * (hr.SENTINEL + 1.0))
    tol = np.stack([ref.bound_hm, ref.bound_hm, ref.bound_gm, ref.bound_h, ref.bound_h,
                    off, off, off], axis=1)
    tol = np.nan_to_num(tol, nan=0.0, posinf=0.0)
    err = np.abs(np.nan_to_num(got) - np.nan_to_num(want))
    err[~np.isfinite(want)] = 0.0
    print(f"RATIO {label} max error / bound {(err[:, 5:8] / np.maximum(tol[:, 5:8], 1e-300)).max():.3f}")
    bad = np.argwhere(err > tol)
    assert bad.size == 0, (label, [(int(i), int(c), got[i, c], want[i, c], err[i, c], tol[i, c])
                                   for i, c in bad[:6]])


@pytest.mark.parametrize("plan,n", CASES, ids=IDS)
def test_ego_form(plan, n):
    """safe_halfspaces on the automatic plan: 16-B loads at the bound, 8-B loads the same bits."""
    assert hr.automatic_geometry(n) == plan and _native.launch_plan(n) == (plan[0], plan[1], 1 << plan[2])
    vec, st = _run_ego(n, False)
    _check(vec, st, ref_ego(n), f"ego {plan} N={n} vec")
    pair, st2 = _run_ego(n, True)
    _check(pair, st2, ref_ego(n), f"ego {plan} N={n} pair")
    same = (vec == pair) | (vec.isnan() & pair.isnan())
    assert bool(same.all()) and torch.equal(st, st2), f"{plan} N={n}: 8-B loads differ from 16-B loads"


@pytest.mark.parametrize("plan,n", CASES, ids=IDS)
def test_given_h_form(plan, n):
    """offsets_given_h on the automatic plan: h echoed, 16-B loads at the bound, 8-B the same bits."""
    assert hr.automatic_geometry(n) == plan
    vec, st = _run_given(n, False)
    _check(vec, st, ref_given(n), f"given-h {plan} N={n} vec")
    np.testing.assert_array_equal(vec.cpu().numpy()[:, 3:5], batch(n)[2])
    pair, st2 = _run_given(n, True)
    _check(pair, st2, ref_given(n), f"given-h {plan} N={n} pair")
    same = (vec == pair) | (vec.isnan() & pair.isnan())
    assert bool(same.all()) and torch.equal(st, st2), f"{plan} N={n}: 8-B loads differ from 16-B loads"


@pytest.mark.parametrize("unaligned", [False, True], ids=["vec", "pair"])
def test_explicit_geometry_with_empty_rows(unaligned):
    """256 x 4 at N = 100: rows 1..3 hold no sample at all and row 0 is partly filled — only the
    predicated form reads nothing past the unit and pads the projections; the records meet the
    reference's bounds as on the automatic 64 x 2 plan."""
    n = 100
    assert n <= 256 * 3 and hr.automatic_geometry(n) == (64, 2, 7)
    got, st = _run_ego(n, unaligned, geometry=(256, 4))
    _check(got, st, ref_ego(n), f"ego 256x4 N={n} {'pair' if unaligned else 'vec'}")
    auto, st2 = _run_ego(n, unaligned)
    _check(auto, st2, ref_ego(n), f"ego automatic N={n} {'pair' if unaligned else 'vec'}")
