"""GPU: the receding-horizon loop (simulation/closed_loop.py) replayed from one graph.

Setup: main.py's multi_obstacle scenario (3 obstacles), the double integrator at DT = 0.2 with
main.py's weights and its input and position bounds (tests/golden/mpc_multi_obstacle_h30.npz),
H = 10, P = 40 rows of straight-line reference and obstacle paths, N = 200 samples, 12 steps.

Yardstick: the ``reference`` backend, which spells one step out with entry points that predate the
loop (index_select of the clamped windows, engine.sampled_halfspaces with a host stream offset,
record_views, filter_batch, the advance arithmetic in torch ops).  ``graph`` (1 and 3 steps per
graph) and ``launches`` must give the same ``states``, ``inputs`` and ``info`` — all ten columns —
BIT FOR BIT: both sides run the same kernels' arithmetic on the same inputs, the halfspace kernel
and the solver are bitwise reproducible, and the advance is copies and one addition.

The fallback branches (steps 3 and 6 of drcvar_mpc_step_advance_f64) are reached with a small
interior-point cap chosen from the reference backend's own info (parent code only), trying
max_iter = 1, 2, 3, ... until its 12 steps hold both solved and unsolved statuses.  Measured on an
MI355X (dr_cvar, with and without the disturbance): caps 1 and 2 leave all 12 steps unsolved;
cap 3 is the first mix, nine unsolved steps (no optimum remembered yet: the reference inputs are
rolled out) and then three solved ones; cap 4 gives solved, seven unsolved, four solved, so the
shifted optimum of step 0 is rolled out and shifted again while it goes stale; from cap 7 every
step is solved.  For the mean metric the first mix is cap 4 (one solved step, then eleven
unsolved).  MIXED_CAPS holds these; the tests assert that both kinds occur at each.  The advance
kernel's own branches are driven without a solver in tests/test_step_advance_gpu.py.

``short_path`` cuts every path to 6 rows, fewer than the H + 1 of a window, so each window is
clamped in every row from the first step on.  It is held to the validity checks and to the
backends' equality only, not to ``solved.all()``: that its QPs solve is no property the loop
promises on a clamped path (on one MI355X all 12 did, in 2 to 5 iterations).

``info`` is finite except where the header defines it otherwise: OBJECTIVE and MAX_SLACK are NaN on
an unsolved step ("optimal only", include/drcvar_mpc.h), and only there.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.config.scenarios import get_scenario_config
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core.mpc_filter import MPCModel
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import obstacles as ob
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.closed_loop import (
    RecedingHorizonFilter)
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.planner import (
    ReferenceTrajectoryPlanner)

pytestmark = pytest.mark.gpu
H, P, N, STEPS, DT = 10, 40, 200, 12, 0.2
SEED, OFFSET = 5, 2 ** 32 - 4          # the 12 steps cross the carry of the stream words
MIXED_CAPS = {"dr_cvar": (3, 4), "mean": (4,)}   # see the module docstring
SOLVED = (_native.MPC_STATUS_OPTIMAL, _native.MPC_STATUS_OPTIMAL_INACCURATE)
VALID = tuple(range(6))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _setup(device, path=P):
    """The model and the first `path` rows of the P-row paths (past its end a path holds its last
    row, so a path shorter than the window is a window clamped in every row)."""
    m = np.load(os.path.join(GOLDEN_DIR, "mpc_multi_obstacle_h30.npz"), allow_pickle=False)
    cfg = get_scenario_config("multi_obstacle")
    model = MPCModel(m["A"], m["B"], m["C"], m["Q"], m["R"], H, tuple(m["u_bounds"]),
                     tuple(m["p_bounds"]), device=device)
    planner = ReferenceTrajectoryPlanner(m["A"], m["B"], m["C"], m["Q"], m["R"], P, DT)
    x_ref, u_ref, _ = planner.straight_line_trajectory(cfg["ego_start"], cfg["ego_goal"])
    nominal = np.stack([ob.generate_nominal_trajectory(o["start"], o["direction"], o["speed"], P, DT)[:P]
                        for o in cfg["obstacles"]])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    x0 = np.zeros(4)
    x0[:2] = cfg["ego_start"]
    disturbance = 1e-2 * np.random.default_rng(3).standard_normal((STEPS, 4))
    return model, to(nominal[:, :path]), to(x_ref[:path]), to(u_ref[:path]), x0, to(disturbance)


def _loop(device, metric="dr_cvar", disturbed=False, steps_per_graph=1, path=P, **kw):
    model, nominal, x_ref, u_ref, _, disturbance = _setup(device, path)
    return RecedingHorizonFilter(model, nominal, x_ref, u_ref, N, RiskParams(), metric=metric,
                                 seed=SEED, disturbance=disturbance if disturbed else None,
                                 steps_per_graph=steps_per_graph, **kw)


def _bytes(result):
    return tuple(t.cpu().numpy().tobytes() for t in result)


@functools.lru_cache(maxsize=None)
def _reference(device, metric, disturbed, step, max_iter, path=P):
    """The reference backend's 12 steps, computed once per configuration: (result on the host,
    its bytes, the per-step solver outputs)."""
    loop = _loop(device, metric, disturbed, path=path, max_iter=max_iter)
    loop.reset(_setup(device)[4], step=step, stream_offset=OFFSET)
    result = tuple(t.cpu() for t in loop.run(STEPS, backend="reference"))
    trace = [tuple(t.cpu() for t in row) for row in loop.reference_trace]
    return result, _bytes(result), trace


def _check_result(result, statuses_mixed=None):
    states, inputs, info = (t.numpy() for t in result)
    assert states.shape == (STEPS + 1, 4) and inputs.shape == (STEPS, 2) and info.shape == (STEPS, 10)
    assert np.isfinite(states).all() and np.isfinite(inputs).all()
    status = info[:, _native.MPC_INFO_STATUS]
    assert np.all(np.isin(status, VALID))
    solved = np.isin(status, SOLVED)
    nan_ok = np.zeros(info.shape, dtype=bool)
    nan_ok[:, [_native.MPC_INFO_OBJECTIVE, _native.MPC_INFO_MAX_SLACK]] = ~solved[:, None]
    assert np.array_equal(np.isnan(info), nan_ok) and np.isfinite(info[~nan_ok]).all()
    if statuses_mixed is not None:
        assert (solved.any() and (~solved).any()) == statuses_mixed, status
    return solved


CONFIGS = {
    "dr_cvar": dict(metric="dr_cvar", disturbed=False, step=0, max_iter=60),
    "mean_disturbed": dict(metric="mean", disturbed=True, step=0, max_iter=60),
    "dr_cvar_disturbed": dict(metric="dr_cvar", disturbed=True, step=0, max_iter=60),
    "past_the_end": dict(metric="dr_cvar", disturbed=False, step=33, max_iter=60),
    "mean_past_the_end": dict(metric="mean", disturbed=True, step=33, max_iter=60),
    "mix_cap3": dict(metric="dr_cvar", disturbed=True, step=0, max_iter=MIXED_CAPS["dr_cvar"][0]),
    "mix_cap4": dict(metric="dr_cvar", disturbed=False, step=0, max_iter=MIXED_CAPS["dr_cvar"][1]),
    "mix_mean": dict(metric="mean", disturbed=True, step=0, max_iter=MIXED_CAPS["mean"][0]),
    # paths of 6 rows < H + 1: every window is clamped from the first step on
    "short_path": dict(metric="dr_cvar", disturbed=False, step=0, max_iter=60, path=6),
}
MIXED = ("mix_cap3", "mix_cap4", "mix_mean")
ANY_STATUS = ("short_path",)   # no statuses are asserted: see the module docstring


@pytest.mark.parametrize("name", list(CONFIGS))
def test_reference_backend_is_a_sound_yardstick(dev, name):
    """Finite, valid statuses, and states[i + 1] = row 1 of step i's solver x (+ the disturbance);
    the capped configurations hold both solved and unsolved steps."""
    c = CONFIGS[name]
    result, _, trace = _reference(dev, **c)
    solved = _check_result(result, statuses_mixed=None if name in ANY_STATUS else name in MIXED)
    states, inputs, info = result
    x0, disturbance = _setup(dev)[4], _setup(dev)[5].cpu()
    assert np.array_equal(states[0].numpy(), x0)
    assert len(trace) == STEPS
    for i, (x, u, inf) in enumerate(trace):
        want = x[1] + disturbance[i] if c["disturbed"] else x[1]
        assert torch.equal(states[i + 1], want), i
        assert torch.equal(inputs[i], u[0]) and inf.numpy().tobytes() == info[i].numpy().tobytes()
    if name not in MIXED and name not in ANY_STATUS:
        assert solved.all()        # the default runs exercise the all-solved path
    if c["step"] == 33:            # the window ran past the paths' end from the first step on
        assert c["step"] + H > P - 1
    if name == "short_path":
        assert c["path"] < H + 1 and _setup(dev, c["path"])[2].shape[0] == c["path"]


@pytest.mark.parametrize("backend,steps_per_graph", [("graph", 1), ("graph", 3), ("launches", 1)])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_backends_equal_the_reference(dev, name, backend, steps_per_graph):
    c = CONFIGS[name]
    _, want, _ = _reference(dev, **c)
    loop = _loop(dev, c["metric"], c["disturbed"], steps_per_graph, path=c.get("path", P),
                 max_iter=c["max_iter"])
    loop.reset(_setup(dev)[4], step=c["step"], stream_offset=OFFSET)
    result = tuple(t.cpu() for t in loop.run(STEPS, backend=backend))
    _check_result(result)
    got = _bytes(result)
    for what, g, w in zip(("states", "inputs", "info"), got, want):
        assert g == w, f"{name} {backend}/{steps_per_graph}: {what} differ"
    # the device state followed: 12 steps on, the offset across 2^32
    assert loop._state.cpu().tolist() == [OFFSET + STEPS, c["step"] + STEPS]


@pytest.mark.parametrize("backend,steps_per_graph", [("graph", 1), ("graph", 3), ("launches", 1),
                                                     ("reference", 1)])
@pytest.mark.parametrize("name", ["dr_cvar_disturbed", "mix_cap4"])
def test_a_second_run_continues_the_first(dev, name, backend, steps_per_graph):
    """6 + 6 steps without a reset in between are the 12 steps; the second run starts where the
    first ended."""
    c = CONFIGS[name]
    whole, _, _ = _reference(dev, **c)
    loop = _loop(dev, c["metric"], c["disturbed"], steps_per_graph, max_iter=c["max_iter"])
    loop.reset(_setup(dev)[4], step=c["step"], stream_offset=OFFSET)
    first = tuple(t.cpu() for t in loop.run(6, backend=backend))
    second = tuple(t.cpu() for t in loop.run(6, backend=backend))
    assert torch.equal(second[0][0], first[0][-1])
    joined = (torch.cat((first[0], second[0][1:])), torch.cat((first[1], second[1])),
              torch.cat((first[2], second[2])))
    assert _bytes(joined) == _bytes(whole)


def test_logs_grow_and_backends_mix(dev):
    """Without a disturbance the logs are rebased when a run outgrows them (the captured step is
    rebuilt), and one loop may change backend between runs: 70 + 2 steps by graph and launches
    end in the state the reference backend reaches in 72."""
    a, b = _loop(dev), _loop(dev)
    x0 = _setup(dev)[4]
    a.reset(x0, stream_offset=OFFSET)
    b.reset(x0, stream_offset=OFFSET)
    sa = a.run(70, backend="graph")[0]
    sa2 = a.run(2, backend="launches")[0]
    sb = b.run(72, backend="reference")[0]
    assert torch.equal(sa, sb[:71]) and torch.equal(sa2, sb[70:])
    assert a._state.cpu().tolist() == b._state.cpu().tolist() == [OFFSET + 72, 72]


def test_run_argument_checks(dev):
    loop = _loop(dev, steps_per_graph=3)
    with pytest.raises(RuntimeError):
        loop.run(3)
    loop.reset(_setup(dev)[4])
    with pytest.raises(ValueError):
        loop.run(4, backend="graph")
    with pytest.raises(ValueError):
        loop.run(3, backend="eager")
    short = _loop(dev, disturbed=True)
    short.reset(_setup(dev)[4])
    with pytest.raises(ValueError):
        short.run(STEPS + 1, backend="launches")      # more steps than disturbance rows
    states, inputs, info = loop.run(0)
    assert states.shape == (1, 4) and inputs.shape == (0, 2) and info.shape == (0, 10)
