"""GPU: the route form of the sampled halfspaces (drcvar_sampled_halfspaces_f64_route,
include/drcvar_loop_route.h) alone.

The defining property, pinned bit for bit: for every problem b the launch writes into that
problem's rows of ``out``, ``status`` and ``selected`` the bytes that
drcvar_sampled_halfspaces_f64_metric (which predates this form and is pinned to the risk-table and
base entries by tests/test_sampled_metric_gpu.py) writes for the unit window ``[b O T, (b + 1) O
T)`` with ``ego_path[b]``, all other arguments equal.  Both sides run the same kernel arithmetic, so
there is no tolerance.  ``out``, ``selected`` and ``status`` sit between guard rows and are filled
with a sentinel before every launch: an unwritten row and a stray write are both seen; the inputs
are compared with their copies after every launch.

The shape is B = 3, O = 2, T = 4, P = 6 with three distinct routes, three different table rows (one
UNBOUNDED) and the metrics mixed inside the launch; one N per plan of the kernel, both noise forms
at the two smallest.
"""
import numpy as np
import pytest
import torch

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskTable

pytestmark = pytest.mark.gpu
SEED = 11
NOISE = {"iso": dict(noise_cov=[[0.01, 0.0], [0.0, 0.01]]), "general": dict(chol=(0.1, 0.05, 0.2))}
SENTINEL, GUARD = -12345.678, 3
B, O, T, P = 3, 2, 4, 6
NAMES = ("mean", "cvar", "dr_cvar")
METRICS = ("mean", "cvar", "dr_cvar")            # (the names the Python layer checks; the codes below
CODE_SETS = ((0, 1, 2), (2, 7, 0))               #  are given through codes=: 7 is no metric)
# problem 1 takes the UNBOUNDED exit (alpha > 1)
TABLE = RiskTable(alpha=[0.2, 1.5, 0.07], delta=[0.1, 0.1, -0.05], epsilon=[0.15, 0.05, 0.3],
                  robot_radius=0.3, obstacle_radius=0.25)
# (offset, step): inside the path, clamped at both ends, past the end, the int64 limits; the offsets
# cross the 2^32 carry of the Philox counter words
STATES = ((2 ** 32 - 1, 0), (2 ** 32, 3), (3, -2), (2 ** 32 - 2, P + 5), (2 ** 32 + 1, -2 ** 63),
          (5, 2 ** 63 - 1))
PLANS = [(20, "iso"), (20, "general"), (200, "iso"), (200, "general"), (1000, "general"),
         (2048, "iso"), (4096, "general"), (8192, "iso"), (16384, "general")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _problem():
    rng = np.random.default_rng(2025)
    nominal = rng.uniform(-5.0, 5.0, size=(B * O, P, 2))
    k = np.arange(P)
    ego = np.stack([np.stack([-7.0 + 0.5 * k, -6.0 + 0.25 * k], axis=1),      # three distinct routes
                    np.stack([6.5 - 0.25 * k, 7.0 + 0.125 * k], axis=1),
                    np.stack([-6.0 + 0.0 * k, 8.0 - 0.5 * k], axis=1)])
    return nominal, ego


def _signed(v):
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _guarded(device, count, width):
    return torch.full((count + 2 * GUARD, width), SENTINEL, dtype=torch.float64, device=device)


def _unguard(t, count, sentinel=SENTINEL):
    a = t.cpu().numpy()
    assert np.all(a[:GUARD] == sentinel) and np.all(a[GUARD + count:] == sentinel), "a write outside"
    got = a[GUARD:GUARD + count]
    assert not np.any(got == sentinel), "an unwritten row"
    return got


def _launch(device, nominal, ego, form, n, noise, D, offset, step, zero_first=True, codes=CODE_SETS[0],
            unit_begin=0, unit_count=None):
    """One launch of ``form`` ("route": ego ``[B, P, 2]``; "metric": ego ``[P, 2]``) between
    guards; ``nominal`` and ``ego`` are device tensors.  Returns (out, status, selected) as numpy."""
    state = torch.tensor([_signed(offset), step], dtype=torch.int64, device=device)
    rows = TABLE.to_device(n, device)
    code_t = torch.tensor(codes, dtype=torch.int32, device=device)
    base = ego._base if ego._base is not None else ego     # the padding of a strided path too
    inputs = (nominal, base, state, rows, code_t)
    before = [t.clone() for t in inputs]
    count = B * O * T - unit_begin if unit_count is None else unit_count
    whole = unit_count is None and unit_begin == 0
    out, sel = _guarded(device, count, 8), _guarded(device, count, 4)
    status = torch.full((count + 2 * GUARD,), -7, dtype=torch.int32, device=device)
    view = lambda t, w: t[GUARD:GUARD + count].view(B * O, T, w) if whole else t[GUARD:GUARD + count]
    kw = dict(draw_period=D, table=rows, codes=code_t, seed=SEED, zero_first_step=zero_first,
              unit_begin=unit_begin, unit_count=unit_count, out=view(out, 8), selected=view(sel, 4),
              status=status[GUARD:GUARD + count], **noise)
    call = engine.sampled_halfspaces_route if form == "route" else engine.sampled_halfspaces_metric
    got_out, got_sel = call(nominal, ego, O, T, n, TABLE, METRICS, state, **kw)
    assert got_out.data_ptr() == out[GUARD:].data_ptr() and got_sel.data_ptr() == sel[GUARD:].data_ptr()
    torch.cuda.synchronize()
    for t, b in zip(inputs, before):                      # the inputs come back unchanged
        assert t.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    return _unguard(out, count), _unguard(status, count, -7), _unguard(sel, count)


def _per_problem(device, nominal, ego, n, noise, D, offset, step, **kw):
    """The three metric launches on the problems' unit windows with ``ego[b]``, concatenated."""
    parts = [_launch(device, nominal, ego[b], "metric", n, noise, D, offset, step,
                     unit_begin=b * O * T, unit_count=O * T, **kw) for b in range(B)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def _same(got, want, what):
    for a, b, name in zip(got, want, ("out", "status", "selected")):
        assert a.tobytes() == b.tobytes(), f"{what}: {name} differs from the per-problem metric launches"


def _tensors(device, strided=False):
    nominal, ego = _problem()
    nominal = torch.from_numpy(nominal).to(device)
    if not strided:
        return nominal, torch.from_numpy(ego).to(device)
    # row stride 3 and a problem stride above P * 3; what lies between the coordinates is NaN
    wide = torch.full((B, P + 2, 3), float("nan"), dtype=torch.float64, device=device)
    wide[:, :P, :2] = torch.from_numpy(ego).to(device)
    path = wide[:, :P, :2]
    assert path.stride() == ((P + 2) * 3, 3, 1)
    return nominal, path


@pytest.mark.parametrize("n,noise", PLANS)
def test_each_problem_is_the_metric_launch_with_its_own_route(dev, n, noise):
    """One N per plan.  At N = 20 and 200: draw periods 1 and 3 x every state x the first step
    noise-free and drawn, the two code sets alternating; above: every state once, the other
    arguments paired with it."""
    nominal, ego = _tensors(dev)
    if n <= 200:
        cases = [(D, state, zero_first) for D in (1, 3) for state in STATES for zero_first in (True, False)]
    else:
        cases = [((1, 3)[k % 2], state, k % 3 != 0) for k, state in enumerate(STATES)]
    seen = set()
    for k, (D, (offset, step), zero_first) in enumerate(cases):
        codes = CODE_SETS[k % 2]
        what = f"N={n} {noise} D={D} offset={offset} step={step} zero_first={zero_first} codes={codes}"
        kw = dict(zero_first=zero_first, codes=codes)
        want = _per_problem(dev, nominal, ego, n, NOISE[noise], D, offset, step, **kw)
        got = _launch(dev, nominal, ego, "route", n, NOISE[noise], D, offset, step, **kw)
        _same(got, want, what)
        status = got[1].reshape(B, O * T)
        assert np.all(status[1] == _native.UNIT_UNBOUNDED) and np.all(status[[0, 2]] == _native.UNIT_OK)
        sel = got[2].reshape(B, O * T, 4)
        for b in range(B):                                 # the unknown code's rows, and only they
            assert np.isnan(sel[b, :, :3]).all() == (codes[b] not in (0, 1, 2)), what
        seen.add(got[0].tobytes())
    assert len(seen) > 1
    # the routes matter: with problem 0's route in every problem the other problems' records differ
    same_route = _launch(dev, nominal, ego[:1].expand(B, P, 2), "route", n, NOISE[noise], 3, 3, 0)
    own_route = _launch(dev, nominal, ego, "route", n, NOISE[noise], 3, 3, 0)
    rows = O * T
    assert same_route[0][:rows].tobytes() == own_route[0][:rows].tobytes()
    assert not np.array_equal(same_route[0][rows:], own_route[0][rows:])


@pytest.mark.parametrize("n", [20, 200])
def test_a_strided_ego_path(dev, n):
    """Row stride 3, problem stride (P + 2) * 3: the dense path's bytes, and the per-problem metric
    launches on the strided rows."""
    nominal, dense = _tensors(dev)
    _, path = _tensors(dev, strided=True)
    for D, (offset, step) in ((1, STATES[1]), (3, STATES[3])):
        want = _launch(dev, nominal, dense, "route", n, NOISE["general"], D, offset, step)
        _same(_launch(dev, nominal, path, "route", n, NOISE["general"], D, offset, step), want, f"N={n}")
        _same(_per_problem(dev, nominal, path, n, NOISE["general"], D, offset, step), want, f"N={n}")


@pytest.mark.parametrize("n", [20, 200, 4096])
def test_problem_stride_zero_is_the_metric_launch(dev, n):
    nominal, ego = _tensors(dev)
    for b, (offset, step) in ((0, STATES[0]), (2, STATES[2])):
        shared = ego[b].expand(B, P, 2)
        assert shared.stride(0) == 0
        want = _launch(dev, nominal, ego[b], "metric", n, NOISE["iso"], 3, offset, step)
        _same(_launch(dev, nominal, shared, "route", n, NOISE["iso"], 3, offset, step), want, f"N={n} b={b}")


@pytest.mark.parametrize("n", [20, 200])
def test_a_unit_window_that_starts_inside_problem_1(dev, n):
    """unit_begin = O T + 3, unit_count = 9: from problem 1's fourth unit into problem 2, rows 0..8
    of out, selected and status and nothing else (the guards)."""
    nominal, ego = _tensors(dev)
    u0, count = O * T + 3, 9
    offset, step = STATES[1]
    whole = _launch(dev, nominal, ego, "route", n, NOISE["general"], 3, offset, step)
    got = _launch(dev, nominal, ego, "route", n, NOISE["general"], 3, offset, step, unit_begin=u0,
                  unit_count=count)
    assert got[0].shape == (count, 8) and got[2].shape == (count, 4)
    _same(got, tuple(a[u0:u0 + count] for a in whole), f"N={n}")
    _same(whole, _per_problem(dev, nominal, ego, n, NOISE["general"], 3, offset, step), f"N={n}")


def test_python_surface(dev):
    nominal, ego = _tensors(dev)
    state = torch.tensor([3, 0], dtype=torch.int64, device=dev)
    out, sel = engine.sampled_halfspaces_route(nominal, ego, O, T, 20, TABLE, METRICS, state, seed=SEED)
    assert tuple(out.shape) == (B * O, T, 8) and tuple(sel.shape) == (B * O, T, 4)
    empty = engine.sampled_halfspaces_route(nominal, ego, O, T, 20, TABLE, METRICS, state, unit_begin=4,
                                            unit_count=0)
    assert tuple(empty[0].shape) == (0, 8) and tuple(empty[1].shape) == (0, 4)
    for bad in (ego[0], ego[:2], ego[:, :P - 1], ego.float(), ego.cpu()):
        with pytest.raises(ValueError, match="ego_path"):
            engine.sampled_halfspaces_route(nominal, bad, O, T, 20, TABLE, METRICS, state)
    with pytest.raises(ValueError, match="names"):
        engine.sampled_halfspaces_route(nominal, ego, O, T, 20, TABLE, METRICS[:-1], state)


def test_graph_replays_follow_the_state(dev):
    """One captured launch, replayed after the state words are changed (a copy on the capture
    stream): every replay gives the eager launch's bytes for the state it then finds."""
    n, D = 200, 3
    versions = [(2 ** 32 - 2 + k, k) for k in range(3)]
    nominal, ego = _tensors(dev)
    rows = TABLE.to_device(n, dev)
    codes = torch.tensor(CODE_SETS[0], dtype=torch.int32, device=dev)
    state = torch.tensor(list(versions[0]), dtype=torch.int64, device=dev)
    out = torch.full((B * O, T, 8), SENTINEL, dtype=torch.float64, device=dev)
    sel = torch.full((B * O, T, 4), SENTINEL, dtype=torch.float64, device=dev)
    status = torch.full((B * O * T,), -7, dtype=torch.int32, device=dev)
    kw = dict(draw_period=D, table=rows, codes=codes, seed=SEED, out=out, selected=sel, status=status,
              **NOISE["iso"])
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):      # the kernel's code object is loaded before the capture
        engine.sampled_halfspaces_route(nominal, ego, O, T, n, TABLE, METRICS, state, stream=stream, **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):     # one stream, no branches
        launch, _, _ = engine.prepare_sampled_halfspaces_route(
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
        _same(got, _per_problem(dev, nominal, ego, n, NOISE["iso"], D, offset, step),
              f"offset {offset}, step {step}")
        seen.append(got[2])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
