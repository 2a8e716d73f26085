"""GPU: the metric form of the sampled halfspaces (drcvar_sampled_halfspaces_f64_metric,
include/drcvar_loop_metric.h) alone.

The defining property, pinned bit for bit: ``out`` and ``status`` are the bytes of
drcvar_sampled_halfspaces_f64_risk (which predates this form and is pinned to the base entry by
tests/test_sampled_risk_gpu.py) for the same arguments, and row r of ``selected`` is the unit's
record columns ``core/mpc_filter.METRIC_COLUMNS`` of its problem's metric followed by +0.0, three
quiet NaNs and +0.0 for a code that is no metric.  Both sides run the same kernel arithmetic, so
there is no tolerance.  ``out``, ``selected`` and ``status`` sit between guard rows and are filled
with a sentinel before every launch: an unwritten row and a stray write are both seen; the inputs
are compared with their copies after every launch.

The shape is the smallest with everything in it: O = 2, T = 3, P = 5, B = 6 with the metrics mixed
inside the launch, table rows that differ per problem (one UNBOUNDED, one DR_UNBOUNDED), N = 20
(one wave) and N = 200 (four waves: the storing lane survives the other waves' return).
"""
import numpy as np
import pytest
import torch

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core.mpc_filter import METRIC_COLUMNS
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskTable

pytestmark = pytest.mark.gpu
SEED = 11
MASK = 2 ** 64 - 1
NOISE = {"iso": dict(noise_cov=[[0.01, 0.0], [0.0, 0.01]]), "general": dict(chol=(0.1, 0.05, 0.2))}
SENTINEL, GUARD = -12345.678, 3
B, O, T, P = 6, 2, 3, 5
NAMES = ("mean", "cvar", "dr_cvar")
CODES = (0, 1, 2, 2, 0, 1)
METRICS = tuple(NAMES[c] for c in CODES)
# problem 3 takes the UNBOUNDED exit (alpha > 1), problem 4 is DR_UNBOUNDED (epsilon < 0)
TABLE = RiskTable(alpha=[0.2, 0.35, 0.07, 1.5, 0.5, 0.9], delta=[0.1, -0.05, 0.0, 0.1, 0.1, -0.05],
                  epsilon=[0.15, 0.0, 0.3, 0.05, -0.1, 0.15], robot_radius=0.3, obstacle_radius=0.25)
STEPS = (0, 3, 9)          # inside the path, clamped rows (3, 4, 4), past the path's end
ZERO = np.zeros(1).tobytes()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _problem():
    rng = np.random.default_rng(2024)
    nominal = rng.uniform(-5.0, 5.0, size=(B * O, P, 2))
    ego = np.stack([-7.0 + 0.5 * np.arange(P), -6.0 + 0.25 * np.arange(P)], axis=1)
    return nominal, ego


def _guarded(device, count, width):
    return torch.full((count + 2 * GUARD, width), SENTINEL, dtype=torch.float64, device=device)


def _unguard(t, count, sentinel=SENTINEL):
    a = t.cpu().numpy()
    assert np.all(a[:GUARD] == sentinel) and np.all(a[GUARD + count:] == sentinel), "a write outside"
    got = a[GUARD:GUARD + count]
    assert not np.any(got == sentinel), "an unwritten row"
    return got


def _launch(device, host, form, n, noise, D, step, zero_first=True, offset=3, unit_begin=0,
            unit_count=None, with_status=True, codes=None):
    """One launch of ``form`` ("metric" or "risk") between guards: (out, status, selected) as numpy
    (status None without one, selected None for the risk form)."""
    nominal, ego = (torch.from_numpy(a).to(device) for a in host)
    state = torch.tensor([offset, step], dtype=torch.int64, device=device)
    rows = TABLE.to_device(n, device)
    code_t = engine.metric_codes(METRICS, B, device) if codes is None else \
        torch.tensor(codes, dtype=torch.int32, device=device)
    inputs = (nominal, ego, state, rows, code_t)
    before = [t.clone() for t in inputs]
    count = B * O * T - unit_begin if unit_count is None else unit_count
    whole = unit_count is None and unit_begin == 0
    out, sel = _guarded(device, count, 8), _guarded(device, count, 4)
    status = torch.full((count + 2 * GUARD,), -7, dtype=torch.int32, device=device)
    view = lambda t, w: t[GUARD:GUARD + count].view(B * O, T, w) if whole else t[GUARD:GUARD + count]
    kw = dict(draw_period=D, table=rows, seed=SEED, zero_first_step=zero_first, unit_begin=unit_begin,
              unit_count=unit_count, out=view(out, 8),
              status=status[GUARD:GUARD + count] if with_status else None, **noise)
    if form == "metric":
        got_out, got_sel = engine.sampled_halfspaces_metric(nominal, ego, O, T, n, TABLE, METRICS, state,
                                                            codes=code_t, selected=view(sel, 4), **kw)
        assert got_out.data_ptr() == out[GUARD:].data_ptr() and got_sel.data_ptr() == sel[GUARD:].data_ptr()
    else:
        engine.sampled_halfspaces_risk(nominal, ego, O, T, n, TABLE, state, **kw)
    torch.cuda.synchronize()
    for t, b in zip(inputs, before):                      # the inputs come back unchanged
        assert t.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    if with_status:
        st = _unguard(status, count, -7)
    else:
        assert np.all(status.cpu().numpy() == -7)
        st = None
    if form == "metric":
        return _unguard(out, count), st, _unguard(sel, count)
    assert np.all(sel.cpu().numpy() == SENTINEL)
    return _unguard(out, count), st, None


def _gather(out, codes=CODES, unit_begin=0):
    """The per-problem column gather of ``out [count, 8]`` (numpy indexing): [count, 3]."""
    want = np.empty((out.shape[0], 3))
    for r in range(out.shape[0]):
        b = (unit_begin + r) // (O * T)
        ch, cg = METRIC_COLUMNS[NAMES[codes[b]]]
        want[r] = out[r, [ch, ch + 1, cg]]
    return want


def _check(got, want, what, codes=CODES, unit_begin=0):
    out, status, sel = got
    assert out.tobytes() == want[0].tobytes(), f"{what}: out differs from the risk-table launch"
    if status is not None:
        assert status.tobytes() == want[1].tobytes(), f"{what}: status {status} != {want[1]}"
    assert np.ascontiguousarray(sel[:, :3]).tobytes() == _gather(out, codes, unit_begin).tobytes(), \
        f"{what}: selected is not the gather of out"
    assert np.ascontiguousarray(sel[:, 3]).tobytes() == ZERO * sel.shape[0], f"{what}: column 3 is not +0.0"


def test_the_codes_are_the_filter_columns():
    assert engine.METRIC_CODES == {name: code for code, name in enumerate(NAMES)}
    assert set(engine.METRIC_CODES) == set(METRIC_COLUMNS) and engine.SELECTED_WIDTH == 4
    assert METRIC_COLUMNS == {"mean": (_native.COL_MEAN_H0, _native.COL_G_MEAN),
                              "cvar": (_native.COL_H0, _native.COL_G_CVAR),
                              "dr_cvar": (_native.COL_H0, _native.COL_G_DR_TILDE)}


@pytest.mark.parametrize("noise", list(NOISE))
@pytest.mark.parametrize("n", [20, 200])
def test_out_is_the_risk_launch_and_selected_its_gather(dev, n, noise):
    """Both plans x both noise forms; inside: the first step noise-free and drawn, draw periods 1, 2
    and B, the state inside the path, on clamped rows and past the end."""
    host = _problem()
    seen = set()
    for zero_first in (True, False):
        for D in (1, 2, B):
            for step in STEPS:
                what = f"N={n} {noise} zero_first={zero_first} D={D} step={step}"
                want = _launch(dev, host, "risk", n, NOISE[noise], D, step, zero_first)
                got = _launch(dev, host, "metric", n, NOISE[noise], D, step, zero_first)
                _check(got, want, what)
                status = got[1].reshape(B, O * T)
                assert np.all(status[3] == _native.UNIT_UNBOUNDED)
                assert np.all(status[4] == _native.UNIT_DR_UNBOUNDED)
                assert np.all(status[[0, 1, 2, 5]] == _native.UNIT_OK)
                seen.add(got[2].tobytes())
    # the gather is of columns that differ: in every OK problem the three offsets are three values
    rec = got[0].reshape(B, O * T, 8)
    for b in (0, 1, 2, 5):
        assert np.all(rec[b, :, 2] != rec[b, :, 5]) and np.all(rec[b, :, 5] != rec[b, :, 7])
    assert len(seen) > 1


def test_a_nan_nominal_row(dev):
    """The non-finite exit stores its row too: problem 1 (cvar) and problem 4 (mean) each hold one
    NaN nominal position in the window."""
    nominal, ego = (a.copy() for a in _problem())
    nominal[1 * O + 1, 1, 0] = float("nan")
    nominal[4 * O + 0, 2, 1] = float("nan")
    for n in (20, 200):
        want = _launch(dev, (nominal, ego), "risk", n, NOISE["general"], 2, 0)
        out, status, sel = _launch(dev, (nominal, ego), "metric", n, NOISE["general"], 2, 0)
        # (a NaN's payload is part of this property: both launches store the same registers)
        _check((out, status, sel), want, f"N={n}")
        hit = np.zeros((B, O, T), dtype=bool)
        hit[1, 1, 1] = hit[4, 0, 2] = True
        st = status.reshape(B, O, T)
        assert np.all(st[hit] & _native.UNIT_NONFINITE) and not np.any(st[~hit] & _native.UNIT_NONFINITE)
        assert np.isnan(sel.reshape(B, O, T, 4)[4, 0, 2, :2]).all()      # the mean of a NaN position


def test_a_unit_window_inside_problems(dev):
    """unit_begin = 5, unit_count = 7: from problem 0's last unit to problem 1's last, rows 0..6 of
    out, selected and status and nothing else (the guards)."""
    host = _problem()
    for n in (20, 200):
        whole = _launch(dev, host, "risk", n, NOISE["iso"], 2, 0)
        got = _launch(dev, host, "metric", n, NOISE["iso"], 2, 0, unit_begin=5, unit_count=7)
        assert got[0].shape == (7, 8) and got[2].shape == (7, 4)
        _check(got, (whole[0][5:12], whole[1][5:12]), f"N={n}", unit_begin=5)
        # problem 0 is "mean", problem 1 "cvar": the window's first row and the rest differ in kind
        assert got[2][0, 2] == got[0][0, 2] and np.all(got[2][1:, 2] == got[0][1:, 5])


def test_without_status(dev):
    host = _problem()
    for n in (20, 200):
        want = _launch(dev, host, "risk", n, NOISE["iso"], B, 3)
        _check(_launch(dev, host, "metric", n, NOISE["iso"], B, 3, with_status=False), want, f"N={n}")


def test_codes_that_are_no_metric(dev):
    """Codes 7 and -1 (given through ``codes=``): NaN triples and +0.0 in those problems' rows, out
    and status byte-equal, every other problem's rows as before."""
    host = _problem()
    codes = [0, 7, 2, -1, 0, 1]       # problem 3 is the UNBOUNDED exit, problem 1 the normal finish
    for n in (20, 200):
        want = _launch(dev, host, "risk", n, NOISE["general"], 2, 0)
        out, status, sel = _launch(dev, host, "metric", n, NOISE["general"], 2, 0, codes=codes)
        assert out.tobytes() == want[0].tobytes() and status.tobytes() == want[1].tobytes()
        sel = sel.reshape(B, O * T, 4)
        good = _gather(out).reshape(B, O * T, 3)
        for b in range(B):
            if codes[b] in (0, 1, 2):
                assert np.ascontiguousarray(sel[b, :, :3]).tobytes() == good[b].tobytes(), b
            else:
                assert np.isnan(sel[b, :, :3]).all(), b
                # quiet NaNs: the top mantissa bit is set
                assert np.all(np.ascontiguousarray(sel[b, :, :3]).view(np.uint64) >> 51 & 1 == 1)
            assert np.ascontiguousarray(sel[b, :, 3]).tobytes() == ZERO * (O * T), b


def test_python_surface(dev):
    host = _problem()
    nominal, ego = (torch.from_numpy(a).to(dev) for a in host)
    state = torch.tensor([3, 0], dtype=torch.int64, device=dev)
    out, sel = engine.sampled_halfspaces_metric(nominal, ego, O, T, 20, TABLE, METRICS, state, seed=SEED)
    assert tuple(out.shape) == (B * O, T, 8) and tuple(sel.shape) == (B * O, T, 4)
    h, g = engine.selected_views(sel, B, O)
    assert tuple(h.shape) == (B, O, T, 2) and tuple(g.shape) == (B, O, T)
    assert h.data_ptr() == sel.data_ptr() and g.data_ptr() == sel.data_ptr() + 16      # views, no copy
    r = out.view(B, O, T, 8)
    for b, name in enumerate(METRICS):
        ch, cg = METRIC_COLUMNS[name]
        assert torch.equal(h[b], r[b, ..., ch:ch + 2]) and torch.equal(g[b], r[b, ..., cg])
    empty = engine.sampled_halfspaces_metric(nominal, ego, O, T, 20, TABLE, METRICS, state, unit_begin=4,
                                             unit_count=0)
    assert tuple(empty[0].shape) == (0, 8) and tuple(empty[1].shape) == (0, 4)
    with pytest.raises(ValueError, match="names"):
        engine.sampled_halfspaces_metric(nominal, ego, O, T, 20, TABLE, METRICS[:-1], state)
    with pytest.raises(ValueError, match="names"):
        engine.sampled_halfspaces_metric(nominal, ego, O, T, 20, TABLE, METRICS[:-1] + ("var",), state)
    with pytest.raises(ValueError, match="codes"):
        engine.sampled_halfspaces_metric(nominal, ego, O, T, 20, TABLE, METRICS, state,
                                         codes=torch.zeros(B + 1, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="selected"):
        engine.sampled_halfspaces_metric(nominal, ego, O, T, 20, TABLE, METRICS, state,
                                         selected=torch.zeros((B * O, T, 8), dtype=torch.float64, device=dev))


def test_graph_replays_follow_the_state(dev):
    """One captured launch, replayed after the state words are changed (a copy on the capture
    stream): every replay gives the eager launch's bytes for the state it then finds."""
    n, D = 200, 2
    host = _problem()
    versions = [(2 ** 32 - 2 + k, k) for k in range(3)]
    nominal, ego = (torch.from_numpy(a).to(dev) for a in host)
    rows, codes = TABLE.to_device(n, dev), engine.metric_codes(METRICS, B, dev)
    state = torch.tensor(list(versions[0]), dtype=torch.int64, device=dev)
    out = torch.full((B * O, T, 8), SENTINEL, dtype=torch.float64, device=dev)
    sel = torch.full((B * O, T, 4), SENTINEL, dtype=torch.float64, device=dev)
    status = torch.full((B * O * T,), -7, dtype=torch.int32, device=dev)
    kw = dict(draw_period=D, table=rows, codes=codes, seed=SEED, out=out, selected=sel, status=status,
              **NOISE["iso"])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):      # the kernel's code object is loaded before the capture
        engine.sampled_halfspaces_metric(nominal, ego, O, T, n, TABLE, METRICS, state, stream=stream, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):     # one stream, no branches
        launch, _, _ = engine.prepare_sampled_halfspaces_metric(
            nominal, ego, O, T, n, TABLE, METRICS, state, stream=torch.cuda.current_stream(dev), **kw)
        launch()
    seen = []
    for offset, step in versions:
        with torch.cuda.stream(stream):
            state.copy_(torch.tensor([offset, step], dtype=torch.int64, device=dev))
            out.fill_(SENTINEL)
            sel.fill_(SENTINEL)
            status.fill_(-7)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = (out.reshape(-1, 8).cpu().numpy(), status.cpu().numpy(), sel.reshape(-1, 4).cpu().numpy())
        eager = _launch(dev, host, "metric", n, NOISE["iso"], D, step, offset=offset)
        for a, b in zip(got, eager):
            assert a.tobytes() == b.tobytes(), f"offset {offset}, step {step}"
        seen.append(got[2])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
