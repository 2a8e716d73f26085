"""GPU: the predicted-ego form of the sampled halfspaces (drcvar_sampled_halfspaces_f64_pred,
include/drcvar_loop_pred.h) alone.

The defining property, pinned bit for bit: for every problem b the record bytes and status words
of its units are those of the base entry (drcvar_sampled_halfspaces_f64, which predates this form)
on the gathered window, with the ego ``[T, 2]`` of problem b

    xs  = x0[b] at t = 0, pred[b, min(t + shift, R - 1)] after it
    ego = c_out xs          an fma chain over the states from +0.0

``unit_begin = b O T``, ``unit_count = O T`` and the state's stream offset.  The ego of the
yardstick is formed here on the host by a multiply-and-add chain in the same order; every c_out
below is a selector or has power-of-two entries, so each product is exact and the chain rounds
where the fma chain rounds: both sides then run the same kernel arithmetic on the same inputs, and
there is no tolerance.  ``out`` and ``status`` sit between guard rows and are filled with a
sentinel before every launch, so an unwritten row and a stray write are both seen.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams

pytestmark = pytest.mark.gpu
SEED = 11
PARAMS = RiskParams(0.3, 0.3, 0.2, 0.1, 0.15)
MASK = 2 ** 64 - 1
ISO_COV = [[0.01, 0.0], [0.0, 0.01]]      # noise_cov: the sampler's isotropic form
GENERAL = (0.1, 0.05, 0.2)                # chol: the general form
NOISE = {"iso": dict(noise_cov=ISO_COV), "general": dict(chol=GENERAL)}
SENTINEL, GUARD = -12345.678, 3           # fill of out; guard rows on either side
EXTRA = 5                                 # path rows past the window


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _signed(v):
    v &= MASK
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _c_out(kind, nx):
    """A selector of the first two states, or a full matrix of signed powers of two."""
    if kind == "selector":
        c = np.zeros((2, nx))
        c[0, 0] = c[1, 1] = 1.0
        return c
    powers = np.array([1.0, -0.5, 0.25, 2.0, -1.0, 0.5, -0.25, 0.125])
    return np.stack([powers[:nx], np.roll(powers, 3)[:nx]])


@functools.lru_cache(maxsize=None)
def _problem(B, O, T, R, nx, seed=0):
    """Host arrays: nominal_path [B O, P, 2], x0 [B, nx], pred [B, R, nx] (P = T + EXTRA)."""
    rng = np.random.default_rng(1000 * seed + 97 * B + 31 * O + 7 * T + 3 * R + nx)
    nominal = rng.uniform(-5.0, 5.0, size=(B * O, T + EXTRA, 2))
    x0 = rng.uniform(-8.0, 8.0, size=(B, nx))
    pred = rng.uniform(-8.0, 8.0, size=(B, R, nx))
    return nominal, x0, pred


def _ego(x0, pred, c, T, shift):
    """[B, T, 2]: the multiply-and-add chain over the states, from +0.0, in the kernel's order."""
    rows = np.minimum(np.arange(T) + shift, pred.shape[1] - 1)
    xs = pred[:, rows, :].copy()
    xs[:, 0, :] = x0
    ego = np.zeros((x0.shape[0], T, 2))
    for j in range(x0.shape[1]):
        ego = ego + xs[:, :, j:j + 1] * c[:, j]
    return ego


def _window_rows(step, T, P):
    return [min(max(step + t, 0), P - 1) for t in range(T)]     # exact integers


def _guarded(device, count):
    out = torch.full((count + 2 * GUARD, 8), SENTINEL, dtype=torch.float64, device=device)
    status = torch.full((count + 2 * GUARD,), -7, dtype=torch.int32, device=device)
    return out, status


def _unguard(out, status, count):
    out, status = out.cpu().numpy(), status.cpu().numpy()
    for rows in (slice(0, GUARD), slice(GUARD + count, None)):
        assert np.all(out[rows] == SENTINEL) and np.all(status[rows] == -7), "a write outside out / status"
    got = out[GUARD:GUARD + count], status[GUARD:GUARD + count]
    assert not np.any(got[0] == SENTINEL) and not np.any(got[1] == -7), "an unwritten record"
    return got


def _base(device, host, c, O, T, n, noise, offset, step, shift, zero_first=True, ego=None):
    """The yardstick: per problem one base-entry call on the gathered window."""
    nominal, x0, pred = host
    B = x0.shape[0]
    rows = torch.tensor(_window_rows(step, T, nominal.shape[1]), device=device)
    window = torch.from_numpy(nominal).to(device).index_select(1, rows)
    ego = _ego(x0, pred, c, T, shift) if ego is None else ego
    records, words = [], []
    for b in range(B):
        out, status = _guarded(device, O * T)
        engine.sampled_halfspaces(window, torch.from_numpy(ego[b]).to(device), n, PARAMS, seed=SEED,
                                  stream_offset=offset & MASK, zero_first_step=zero_first,
                                  unit_begin=b * O * T, unit_count=O * T, out=out[GUARD:GUARD + O * T],
                                  status=status[GUARD:GUARD + O * T], **noise)
        r, s = _unguard(out, status, O * T)
        records.append(r)
        words.append(s)
    return np.concatenate(records), np.concatenate(words)


def _pred_form(device, host, c, O, T, n, noise, offset, step, shift, zero_first=True, unit_begin=0,
               unit_count=None):
    nominal, x0, pred = (torch.from_numpy(a).to(device) for a in host)
    state = torch.tensor([_signed(offset), step], dtype=torch.int64, device=device)
    before = [t.clone() for t in (nominal, x0, pred, state)]
    total = nominal.shape[0] * T
    count = total - unit_begin if unit_count is None else unit_count
    out, status = _guarded(device, count)
    view = out[GUARD:GUARD + count]
    if unit_count is None and unit_begin == 0:
        view = view.view(nominal.shape[0], T, 8)
    got = engine.sampled_halfspaces_pred(nominal, x0, pred, c, O, T, n, PARAMS, state, shift=shift,
                                         seed=SEED, zero_first_step=zero_first, unit_begin=unit_begin,
                                         unit_count=unit_count, out=view,
                                         status=status[GUARD:GUARD + count], **noise)
    assert got.data_ptr() == view.data_ptr()
    for t, b in zip((nominal, x0, pred, state), before):      # the inputs come back unchanged
        assert t.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    return _unguard(out, status, count)


def _same(got, want, what):
    assert got[1].tobytes() == want[1].tobytes(), f"{what}: status {got[1]} != {want[1]}"
    assert got[0].tobytes() == want[0].tobytes(), \
        f"{what}: rows {np.nonzero(np.any(got[0] != want[0], axis=1))[0]} differ"


@pytest.mark.parametrize("n", [20, 200, 1000, 2048, 4096, 8192, 16384])
def test_every_plan_and_both_noise_forms(dev, n):
    host = _problem(2, 3, 4, 5, 4)
    c = _c_out("selector", 4)
    for name, noise in NOISE.items():
        got = _pred_form(dev, host, c, 3, 4, n, noise, 3, 1, 1)
        _same(got, _base(dev, host, c, 3, 4, n, noise, 3, 1, 1), f"N={n} {name}")
        assert np.all(got[1] == _native.UNIT_OK)


def test_problems_windows_rows_states_and_shift(dev):
    """B x O x T x pred_rows x shift in full, the state count, c_out and the noise form cycling
    through: every index rule (the problem of a unit, the clamp of the prediction row, t = 0)."""
    kinds = itertools.cycle(itertools.product((2, 4, 8), ("selector", "powers"), ("iso", "general")))
    cases = 0
    for B, O, T in itertools.product((1, 2, 5), (1, 3), (1, 4, 10)):
        for R in sorted({1, T, T + 1}):
            for shift in (0, 1):
                nx, kind, noise = next(kinds)
                host, c = _problem(B, O, T, R, nx), _c_out(kind, nx)
                what = f"B={B} O={O} T={T} R={R} shift={shift} nx={nx} {kind} {noise}"
                _same(_pred_form(dev, host, c, O, T, 20, NOISE[noise], 3, 2, shift),
                      _base(dev, host, c, O, T, 20, NOISE[noise], 3, 2, shift), what)
                cases += 1
    assert cases == 96
    # the clamp and the shift are seen by the yardstick: different rows give different egos
    x0, pred = _problem(2, 1, 4, 5, 4)[1:]
    c = _c_out("powers", 4)
    assert not np.array_equal(_ego(x0, pred, c, 4, 0), _ego(x0, pred, c, 4, 1))
    assert not np.array_equal(_ego(x0, pred[:, :3], c, 4, 1), _ego(x0, pred, c, 4, 1))


@pytest.mark.parametrize("kind", ["selector", "powers"])
def test_unit_windows(dev, kind):
    """Windows that start and end inside different problems (B = 5, O = 3, T = 4: 12 units each)."""
    B, O, T, nx = 5, 3, 4, 8
    host, c = _problem(B, O, T, T, nx), _c_out(kind, nx)
    whole = _base(dev, host, c, O, T, 1000, NOISE["general"], 3, 2, 1)
    _same(_pred_form(dev, host, c, O, T, 1000, NOISE["general"], 3, 2, 1), whole, "whole")
    for u0, count in ((5, 20), (13, 30), (23, 2), (59, 1), (0, 12), (47, 13)):
        got = _pred_form(dev, host, c, O, T, 1000, NOISE["general"], 3, 2, 1, unit_begin=u0, unit_count=count)
        assert got[0].shape == (count, 8)
        _same(got, (whole[0][u0:u0 + count], whole[1][u0:u0 + count]), f"units {u0}..{u0 + count - 1}")
    tail = _pred_form(dev, host, c, O, T, 1000, NOISE["general"], 3, 2, 1, unit_begin=50)
    _same(tail, (whole[0][50:], whole[1][50:]), "units 50..")
    # nothing to launch
    nominal, x0, pred = (torch.from_numpy(a).to(dev) for a in host)
    state = torch.tensor([3, 2], dtype=torch.int64, device=dev)
    empty = engine.sampled_halfspaces_pred(nominal, x0, pred, c, O, T, 1000, PARAMS, state, unit_begin=17,
                                           unit_count=0)
    assert tuple(empty.shape) == (0, 8)


# window starts: inside, partly and fully clamped, before the path, and the ends of the int64 range
STEPS = (0, 2, 7, 40, -3, 2 ** 63 - 1, -2 ** 63)
OFFSETS = (3, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5)


@pytest.mark.parametrize("name", list(NOISE))
def test_steps_and_offsets(dev, name):
    host, c = _problem(2, 3, 4, 5, 4), _c_out("powers", 4)
    for step in STEPS:
        for offset in OFFSETS:
            _same(_pred_form(dev, host, c, 3, 4, 1000, NOISE[name], offset, _signed(step), 1),
                  _base(dev, host, c, 3, 4, 1000, NOISE[name], offset, _signed(step), 1),
                  f"step={step} offset={offset}")
    # the offsets on either side of the carry are different draws
    a = _base(dev, host, c, 3, 4, 1000, NOISE[name], 2 ** 32 - 1, 2, 1)[0].reshape(6, 4, 8)
    b = _base(dev, host, c, 3, 4, 1000, NOISE[name], 2 ** 32, 2, 1)[0].reshape(6, 4, 8)
    assert np.all(a[:, 1:, 5] != b[:, 1:, 5])


def test_zero_first_step_on_and_off(dev):
    host, c = _problem(2, 3, 4, 5, 4), _c_out("selector", 4)
    on = _pred_form(dev, host, c, 3, 4, 1000, NOISE["iso"], 3, 2, 1)
    off = _pred_form(dev, host, c, 3, 4, 1000, NOISE["iso"], 3, 2, 1, zero_first=False)
    _same(on, _base(dev, host, c, 3, 4, 1000, NOISE["iso"], 3, 2, 1), "noise-free first step")
    _same(off, _base(dev, host, c, 3, 4, 1000, NOISE["iso"], 3, 2, 1, zero_first=False), "every step drawn")
    on, off = on[0].reshape(6, 4, 8), off[0].reshape(6, 4, 8)
    assert np.all(on[:, 0, 5] != off[:, 0, 5]) and on[:, 1:].tobytes() == off[:, 1:].tobytes()
    # the noise-free unit does not depend on the offset, every other unit does
    other = _pred_form(dev, host, c, 3, 4, 1000, NOISE["iso"], 4, 2, 1)[0].reshape(6, 4, 8)
    assert on[:, 0].tobytes() == other[:, 0].tobytes() and np.all(on[:, 1:, 5] != other[:, 1:, 5])


def test_records_follow_the_ego(dev):
    O, T, nx = 3, 4, 4
    nominal, x0, pred = (a.copy() for a in _problem(2, O, T, T + 1, nx))
    c = _c_out("selector", nx)
    # (a) one launch, a zero noise factor (every sample is the nominal point, so a unit's record
    # depends on its nominal row and its ego alone): two problems with equal nominal paths and
    # equal pred but different x0 differ at t = 0 and agree at t >= 1
    nominal[O:] = nominal[:O]
    pred[1] = pred[0]
    zero = dict(chol=(0.0, 0.0, 0.0))
    got = _pred_form(dev, (nominal, x0, pred), c, O, T, 20, zero, 3, 2, 1, zero_first=False)
    _same(got, _base(dev, (nominal, x0, pred), c, O, T, 20, zero, 3, 2, 1, zero_first=False), "zero factor")
    rec = got[0].reshape(2, O, T, 8)
    assert np.all(rec[0, :, 0, 3:5] != rec[1, :, 0, 3:5])
    assert rec[0, :, 1:].tobytes() == rec[1, :, 1:].tobytes()
    # (b) drawn samples: moving problem 1's x0 changes its t = 0 units and nothing else
    a = _pred_form(dev, (nominal, x0, pred), c, O, T, 1000, NOISE["general"], 3, 2, 1)[0].reshape(2, O, T, 8)
    moved = x0.copy()
    moved[1, :2] += [0.5, -0.25]
    b = _pred_form(dev, (nominal, moved, pred), c, O, T, 1000, NOISE["general"], 3, 2, 1)[0].reshape(2, O, T, 8)
    assert a[0].tobytes() == b[0].tobytes() and a[1, :, 1:].tobytes() == b[1, :, 1:].tobytes()
    assert np.all(a[1, :, 0, 3:6] != b[1, :, 0, 3:6])
    # ... and moving one prediction row changes the units of that row alone
    bent = pred.copy()
    bent[0, 3, :2] += [0.5, 0.25]                      # shift = 1: row 3 is window step t = 2
    d = _pred_form(dev, (nominal, x0, bent), c, O, T, 1000, NOISE["general"], 3, 2, 1)[0].reshape(2, O, T, 8)
    differs = np.any(a != d, axis=3)
    want = np.zeros((2, O, T), dtype=bool)
    want[0, :, 2] = True
    assert np.array_equal(differs, want)


def test_reference_window_gives_the_device_state_form(dev):
    """x0 and pred set to the reference window (two states, c_out = I): the records are
    sampled_halfspaces_dev's on that ego path, bit for bit."""
    B, O, T, step = 2, 3, 4, 2
    nominal = _problem(B, O, T, T + 1, 2)[0]
    P = nominal.shape[1]
    ego_path = np.stack([-7.0 + 0.5 * np.arange(P), -6.0 + 0.25 * np.arange(P)], axis=1)
    x0 = np.broadcast_to(ego_path[step], (B, 2)).copy()
    pred = np.broadcast_to(ego_path[_window_rows(step - 1, T + 1, P)], (B, T + 1, 2)).copy()
    for name, noise in NOISE.items():
        got = _pred_form(dev, (nominal, x0, pred), np.eye(2), O, T, 1000, noise, 2 ** 32 - 1, step, 1)
        state = torch.tensor([2 ** 32 - 1, step], dtype=torch.int64, device=dev)
        status = torch.full((B * O * T,), -7, dtype=torch.int32, device=dev)
        want = engine.sampled_halfspaces_dev(torch.from_numpy(nominal).to(dev), torch.from_numpy(ego_path).to(dev),
                                             T, 1000, PARAMS, state, seed=SEED, status=status, **noise)
        _same(got, (want.reshape(-1, 8).cpu().numpy(), status.cpu().numpy()), name)


def test_a_nan_row_stays_in_its_problem(dev):
    B, O, T, nx = 3, 3, 4, 4
    nominal, x0, pred = (a.copy() for a in _problem(B, O, T, T + 1, nx))
    c = _c_out("powers", nx)
    clean = _pred_form(dev, (nominal, x0, pred), c, O, T, 1000, NOISE["general"], 3, 2, 1)
    pred[1, 2, 1] = float("nan")                       # shift = 1: window step t = 1 of problem 1
    got = _pred_form(dev, (nominal, x0, pred), c, O, T, 1000, NOISE["general"], 3, 2, 1)
    # the way a non-finite ego flows through the base entry: the same status words, NaN where it
    # has NaN (a NaN's payload is not part of the property) and the same bytes everywhere else
    want = _base(dev, (nominal, x0, pred), c, O, T, 1000, NOISE["general"], 3, 2, 1)
    assert got[1].tobytes() == want[1].tobytes()
    nan = np.isnan(want[0])
    assert np.array_equal(np.isnan(got[0]), nan) and got[0][~nan].tobytes() == want[0][~nan].tobytes()
    a, b = clean[0].reshape(B, O, T, 8), got[0].reshape(B, O, T, 8)
    differs = np.any(a.view(np.uint64) != b.view(np.uint64), axis=3)
    want = np.zeros((B, O, T), dtype=bool)
    want[1, :, 1] = True
    assert np.array_equal(differs, want)
    assert np.isnan(b[1, :, 1, 3:5]).all() and np.isfinite(b[differs == 0]).all()
    sa, sb = clean[1].reshape(B, O, T), got[1].reshape(B, O, T)
    assert np.array_equal(sa[~want], sb[~want])


def test_graph_replays_follow_x0_pred_and_state(dev):
    """One captured launch; x0, pred and state are rewritten on the device between replays (copies
    on the capture stream), and every replay is the base entry on what they then hold."""
    B, O, T, nx, n = 2, 3, 4, 4, 1000
    c = _c_out("powers", nx)
    versions = [(_problem(B, O, T, T + 1, nx, seed=k), 2 ** 32 - 2 + k, 1 + k) for k in range(3)]
    nominal = torch.from_numpy(versions[0][0][0]).to(dev)
    x0 = torch.from_numpy(versions[0][0][1]).to(dev)
    pred = torch.from_numpy(versions[0][0][2]).to(dev)
    state = torch.tensor([versions[0][1], versions[0][2]], dtype=torch.int64, device=dev)
    out = torch.full((B * O, T, 8), SENTINEL, dtype=torch.float64, device=dev)
    status = torch.full((B * O * T,), -7, dtype=torch.int32, device=dev)
    kw = dict(shift=1, seed=SEED, out=out, status=status, **NOISE["iso"])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):      # the kernel's code object is loaded before the capture
        engine.sampled_halfspaces_pred(nominal, x0, pred, c, O, T, n, PARAMS, state, stream=stream, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):     # one stream, no branches
        launch, _ = engine.prepare_sampled_halfspaces_pred(nominal, x0, pred, c, O, T, n, PARAMS, state,
                                                           stream=torch.cuda.current_stream(dev), **kw)
        launch()
    seen = []
    for (host, offset, step) in versions:
        with torch.cuda.stream(stream):
            x0.copy_(torch.from_numpy(host[1]).to(dev))
            pred.copy_(torch.from_numpy(host[2]).to(dev))
            state.copy_(torch.tensor([offset, step], dtype=torch.int64, device=dev))
            out.fill_(SENTINEL)
            status.fill_(-7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = (out.reshape(-1, 8).cpu().numpy(), status.cpu().numpy())
        want = _base(dev, (versions[0][0][0], host[1], host[2]), c, O, T, n, NOISE["iso"], offset, step, 1)
        _same(got, want, f"replay at offset {offset}, step {step}")
        seen.append(got[0])
    assert np.all(np.any(seen[0] != seen[1], axis=1)) and np.all(np.any(seen[1] != seen[2], axis=1))
