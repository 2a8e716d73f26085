"""GPU: the fused halfspace kernel's order statistic on every compiled form.

Every unit of every launch is compared with the long-double reference of
tests/halfspace_reference.py at the unit's own derived rounding bound (1e-14 .. 1e-10, never the
1e-6 of the parity tests), on units whose tau has weight one half in L and a planted gap around it
(so a rank off by one is hundreds of bounds away, tests/test_halfspace_reference.py), over the
families that leave the fast path on purpose (tau below / above the window, a crowded bucket, no
window variance), on all 14 launch geometries and the streaming kernel, with `ego` and with a given
`h`, through 16-B, 8-B (unaligned buffer) and nontemporal (> 256 MiB launch) loads.  Sentinel / NaN
positions and status words must be exact.

Each test prints `RATIO <form> <family> <max error / bound>`; docs/lab_notebook.md §6b records them.
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
STREAM = ("stream",)
AUTOMATIC = hr.GEOMETRIES[:hr.N_AUTOMATIC]
N_CLASSES = len(hr.A0)


def _sizes(form):
    return hr.STREAM_SIZES if form == STREAM else hr.sizes_of(form[0], form[1])


def _head(form):
    return hr.STREAM_BLOCK if form == STREAM else hr.head_of(form[0], form[1])


def _automatic_sizes(form):
    """The sizes of a form that the automatic chain (the only one the given-h entry has) runs on
    that form."""
    if form == STREAM:
        return hr.STREAM_SIZES
    return [n for n in _sizes(form) if hr.automatic_geometry(n) == form]


def _params(alpha, epsilon=hr.EPSILON):
    return RiskParams(hr.RR, hr.RO, alpha, hr.DELTA, epsilon)


def _slim(ref):
    return dict(rec=ref.rec, bound=ref.bound, bound_h=ref.bound_h, bound_hm=ref.bound_hm,
                bound_gm=ref.bound_gm, ok=ref.ok)


@functools.lru_cache(maxsize=None)
def _ref_safe(n, ac, head):
    blk = hr.cases(n, ac, 0, head)
    return _slim(hr.reference(blk["samples"], ego=blk["ego"], alpha=blk["alpha"]))


@functools.lru_cache(maxsize=None)
def _ref_given(n, ac, head):
    names, s, h = hr.given_h_cases(hr.cases(n, ac, 0, head))
    return names, _slim(hr.reference(s, h=h, alpha=hr.cases(n, ac, 0, head)["alpha"]))


def _device(a, unaligned=False):
    """`a` on the device; unaligned: its base 8 bytes past 16-byte alignment (the 8-B load form)."""
    t = torch.as_tensor(np.ascontiguousarray(a))
    if not unaligned:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=torch.float64, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8
    return v


def _run_safe(samples, ego, params, geometry=None, unaligned=False, plain=False):
    """samples [U, N, 2], ego [U, 2] -> (records [U, 8], status [U]); O = 1, the units along T."""
    s = samples if torch.is_tensor(samples) else _device(samples[None], unaligned)
    e = ego if torch.is_tensor(ego) else _device(ego)
    status = torch.full((s.shape[1],), -1, dtype=torch.int32, device=DEV)
    if plain:
        out = engine.safe_halfspaces(s, e, params, status=status)
    else:
        launch, out = engine.prepare_safe_halfspaces(s, e, params, geometry=geometry, status=status)
        launch()
    return out[0], status


def _run_given(samples, h, params, unaligned=False):
    s = samples if torch.is_tensor(samples) else _device(samples, unaligned)
    hh = h if torch.is_tensor(h) else _device(h)
    status = torch.full((s.shape[0],), -1, dtype=torch.int32, device=DEV)
    return engine.offsets_given_h(s, hh, params, status=status), status


RATIOS = {}


def _check(got, ref, names, label, form):
    """Records `got` [U, 8] against the reference at the units' bounds; NaN and sentinel positions
    exact.  Failing units (ref['ok'] false) hold exact sentinels: 100, 100, 100 - R_c |h|."""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    want = ref["rec"]
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=label)
    for c in (5, 6):
        np.testing.assert_array_equal(got[:, c] == hr.SENTINEL, want[:, c] == hr.SENTINEL, err_msg=label)
    off = np.where(ref["ok"], np.nan_to_num(ref["bound"]), 4 * hr.U64 * (hr.SENTINEL + 1.0))
    tol = np.stack([ref["bound_hm"], ref["bound_hm"], ref["bound_gm"], ref["bound_h"], ref["bound_h"],
                    off, off, off], axis=1)
    tol = np.nan_to_num(tol, nan=0.0, posinf=0.0)
    err = np.abs(np.nan_to_num(got) - np.nan_to_num(want))
    err[~np.isfinite(want)] = 0.0
    for i, name in enumerate(names):
        r = float((err[i, 5:8] / np.maximum(tol[i, 5:8], 1e-300)).max())
        key = (str(form), name)
        RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    bad = np.argwhere(err > tol)
    assert bad.size == 0, (label, [(names[i], int(c), got[i, c], want[i, c], err[i, c], tol[i, c])
                                   for i, c in bad[:6]])


def _report(form):
    for (f, name), r in sorted(RATIOS.items()):
        if f == str(form):
            print(f"RATIO {f} {name} {r:.3f}")


FORMS = hr.GEOMETRIES + [STREAM]


@pytest.mark.parametrize("unaligned", [False, True], ids=["vec", "pair"])
@pytest.mark.parametrize("form", FORMS, ids=str)
def test_safe_halfspaces_every_form(form, unaligned):
    """The whole case block, every alpha class, every size of the form, through the explicit
    geometry (and, where the automatic chain picks the same form, through the plain entry: the same
    kernel, so bit for bit).  pair: the same from a buffer 8 bytes past 16-byte alignment — the
    8-B load form (`VEC = false` on the streaming kernel), whose records equal the aligned
    launch's bit for bit."""
    geometry = None if form == STREAM else form[:2]
    for n in _sizes(form):
        for ac in range(N_CLASSES):
            blk = hr.cases(n, ac, 0, _head(form))
            ref = _ref_safe(n, ac, _head(form))
            label = f"{form} N={n} a0={hr.A0[ac]} {'pair' if unaligned else 'vec'}"
            got, status = _run_safe(blk["samples"], blk["ego"], _params(blk["alpha"]), geometry, unaligned)
            _check(got, ref, blk["names"], label, form)
            assert (status == _native.UNIT_OK).all(), label
            if form == STREAM or hr.automatic_geometry(n) == form:
                plain, st2 = _run_safe(blk["samples"], blk["ego"], _params(blk["alpha"]), None, unaligned,
                                       plain=True)
                assert torch.equal(plain, got) and torch.equal(st2, status), label
            if unaligned:
                vec, _ = _run_safe(blk["samples"], blk["ego"], _params(blk["alpha"]), geometry, False)
                assert torch.equal(vec, got), f"{label}: 8-B loads differ from 16-B loads"
    _report(form)


@pytest.mark.parametrize("unaligned", [False, True], ids=["vec", "pair"])
@pytest.mark.parametrize("form", AUTOMATIC + [STREAM], ids=str)
def test_offsets_given_h_every_form(form, unaligned):
    """The same units with the reference's h fed to offsets_given_h (+ h = 0, |h| = 1e-3, 1e3):
    against the reference at the bound, h echoed exactly, and within the sum of the bounds of the
    safe_halfspaces launch of the same units."""
    for n in _automatic_sizes(form):
        for ac in range(N_CLASSES):
            blk = hr.cases(n, ac, 0, _head(form))
            names, s, h = hr.given_h_cases(blk)
            _, ref = _ref_given(n, ac, _head(form))
            label = f"given-h {form} N={n} a0={hr.A0[ac]} {'pair' if unaligned else 'vec'}"
            got, status = _run_given(s, h, _params(blk["alpha"]), unaligned)
            _check(got, ref, names, label, ("given-h",) + tuple(form))
            assert (status == _native.UNIT_OK).all(), label
            g = got.cpu().numpy()
            np.testing.assert_array_equal(g[:, 3:5], h, err_msg=label)
            safe, _ = _run_safe(blk["samples"], blk["ego"], _params(blk["alpha"]))
            rs = _ref_safe(n, ac, _head(form))
            U = len(blk["names"])
            d = np.abs(g[:U, 5:8] - safe.cpu().numpy()[:, 5:8])
            assert (d <= (ref["bound"][:U] + rs["bound"])[:, None]).all(), label
            if unaligned:
                vec, _ = _run_given(s, h, _params(blk["alpha"]), False)
                assert torch.equal(vec, got), f"{label}: 8-B loads differ from 16-B loads"
    _report(("given-h",) + tuple(form))


@pytest.mark.parametrize("form", AUTOMATIC, ids=str)
def test_nontemporal_loads_every_plan(form):
    """A launch reading just over 256 MiB takes the nontemporal load form: the case block tiled on
    the device; every replica's record equals, bit for bit, the record of the same unit from the
    small 16-B-load launch (which test_safe_halfspaces_every_form checks against the reference) —
    the two forms differ only in the load instruction.  Both entries; steps / units on grid x."""
    n = form[0] * (form[1] - 1) + 1
    try:
        for ac in range(N_CLASSES):
            blk = hr.cases(n, ac, 0, _head(form))
            names, sh, h = hr.given_h_cases(blk)
            p = _params(blk["alpha"])
            for entry in ("safe", "given"):
                small_s = _device(blk["samples"] if entry == "safe" else sh)
                small_d = _device(blk["ego"] if entry == "safe" else h)
                U = small_s.shape[0]
                reps = ((256 << 20) // (U * n * 16)) + 1
                big_s, big_d = small_s.repeat(reps, 1, 1), small_d.repeat(reps, 1)
                assert big_s.shape[0] * n * 16 > 256 << 20 and big_s.data_ptr() % 16 == 0
                if entry == "safe":
                    small, _ = _run_safe(small_s[None], small_d, p)
                    big, status = _run_safe(big_s[None], big_d, p)
                else:
                    small, _ = _run_given(small_s, small_d, p)
                    big, status = _run_given(big_s, big_d, p)
                same = (big.view(reps, U, 8) == small[None]) | (big.view(reps, U, 8).isnan() & small[None].isnan())
                assert bool(same.all()), f"nontemporal {entry} {form} N={n} a0={hr.A0[ac]}"
                assert (status == _native.UNIT_OK).all()
                del big_s, big_d, big, status, same
    finally:
        torch.cuda.empty_cache()


@pytest.mark.parametrize("form", AUTOMATIC, ids=str)
def test_order_independence(form):
    """A random permutation and the two sorted orders of the planted Gaussian and bimodal units:
    offsets within the sum of the bounds of the unpermuted unit's, the direction moves only by
    summation order."""
    rng = np.random.default_rng(form[0] * 100 + form[1])
    for n in _automatic_sizes(form):
        for ac in range(N_CLASSES):
            blk = hr.cases(n, ac, 0, _head(form))
            ref = _ref_safe(n, ac, _head(form))
            pick = [blk["names"].index(f) for f in ("gauss", "bimodal30", "bimodal10")]
            base, _ = _run_safe(blk["samples"], blk["ego"], _params(blk["alpha"]))
            base = base.cpu().numpy()[pick]
            s = blk["samples"][pick]
            d = np.einsum("unc,uc->un", s, ref["rec"][pick, 3:5])
            for order in (rng.permuted(np.tile(np.arange(n), (len(pick), 1)), axis=1),
                          np.argsort(d, axis=1), np.argsort(-d, axis=1)):
                sp = np.take_along_axis(s, order[:, :, None], axis=1)
                got, _ = _run_safe(sp, blk["ego"][pick], _params(blk["alpha"]))
                got = got.cpu().numpy()
                label = f"{form} N={n} a0={hr.A0[ac]}"
                assert (np.abs(got[:, 5:8] - base[:, 5:8]) <= 2 * ref["bound"][pick, None]).all(), label
                assert (np.abs(got[:, 3:5] - base[:, 3:5]) <= 2 * ref["bound_h"][pick, None]).all(), label


def _failure_units(n, head):
    blk = hr.cases(n, 2, 0, head)
    g = blk["names"].index("gauss")
    s = np.repeat(blk["samples"][g:g + 1], 3, axis=0)
    s[1, n - 1, 1] = np.nan            # the last valid sample of the last row
    s[2, n // 2, 0] = np.inf
    return ["clean", "nan_last", "inf_mid"], s, np.repeat(blk["ego"][g:g + 1], 3, axis=0), blk["alpha"]


@pytest.mark.parametrize("form", FORMS, ids=str)
def test_failure_words_every_form(form):
    """Status words and sentinel columns, exactly, on every geometry and on the given-h forms: a
    NaN in the last valid sample of the last row, a +inf, alpha > 1, epsilon < 0."""
    n = _sizes(form)[0] if form == STREAM else form[0] * (form[1] - 1) + 1
    names, s, ego, alpha = _failure_units(n, _head(form))
    nonfinite = np.array([0, 1, 1]) * _native.UNIT_NONFINITE
    h = hr.reference(s[:1], ego=ego[:1], alpha=alpha).rec[[0, 0, 0], 3:5]
    for a, eps, bits in [(alpha, hr.EPSILON, 0), (1.5, hr.EPSILON, _native.UNIT_UNBOUNDED),
                         (alpha, -0.1, _native.UNIT_DR_UNBOUNDED)]:
        label = f"{form} N={n} alpha={a} eps={eps}"
        geometry = None if form == STREAM else form[:2]
        got, status = _run_safe(s, ego, _params(a, eps), geometry)
        ref = _slim(hr.reference(s, ego=ego, alpha=a, epsilon=eps))
        _check(got, ref, names, label, ("failure",))
        np.testing.assert_array_equal(status.cpu().numpy(), nonfinite | bits, err_msg=label)
        g = got.cpu().numpy()
        assert (g[:, 5] == hr.SENTINEL).tolist() == [bits == _native.UNIT_UNBOUNDED, True, True], label
        assert (g[:, 6] == hr.SENTINEL).tolist() == [bits != 0, True, True], label
        if form == STREAM or hr.automatic_geometry(n) == form:
            got, status = _run_given(s, h, _params(a, eps))
            ref = _slim(hr.reference(s, h=h, alpha=a, epsilon=eps))
            _check(got, ref, names, "given-h " + label, ("failure",))
            np.testing.assert_array_equal(status.cpu().numpy(), nonfinite | bits, err_msg=label)
