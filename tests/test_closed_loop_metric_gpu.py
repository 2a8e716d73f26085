"""GPU: a batch of receding-horizon loops with a metric per problem (simulation/closed_loop.py,
RecedingHorizonBatch(metric=[...]); the halfspace launch is drcvar_sampled_halfspaces_f64_metric,
include/drcvar_loop_metric.h).

Setup: that of tests/test_closed_loop_batch_gpu.py, imported (main.py's multi_obstacle scenario,
H = 10, P = 40, N = 20, 12 steps from stream offset 2^32 - 4) with B = 6 problems: the 3 metrics x
D = 2 replicates, problem b = s D + r, every problem with a start of its own.

Yardstick: the ``reference`` backend, which spells the metric form out with what predates it — the
per-problem records of the risk-table batch's reference, each problem's METRIC_COLUMNS gathered
with torch indexing, then one filter_batch of all B problems.  ``graph`` (1 and 3 steps per graph)
and ``launches`` must give the same states, inputs and info — all ten columns — BIT FOR BIT.
"""
import functools

import numpy as np
import pytest
import torch

import test_closed_loop_batch_gpu as base
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams, RiskTable
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.closed_loop import (
    LoopEvaluation, RecedingHorizonBatch)

pytestmark = pytest.mark.gpu
STEPS, OFFSET, N, SEED, H = base.STEPS, base.OFFSET, base.N, base.SEED, base.H
BACKENDS, SOLVED = base.BACKENDS, base.SOLVED
NAMES = ("mean", "cvar", "dr_cvar")
S, D = 3, 2
B = S * D
METRICS = tuple(name for name in NAMES for _ in range(D))                # b = s D + r
TENSORS = ("min_clearance", "collided", "step_hits", "step_collision_rate")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _batch(device, metric=METRICS, params=None, disturbed=False, steps_per_graph=1, n_problems=B, **kw):
    model, nominal, x_ref, u_ref = base._setup(device)
    params = RiskParams() if params is None else params
    if not isinstance(metric, str):
        kw.setdefault("draw_period", D)
    return RecedingHorizonBatch(model, nominal, x_ref, u_ref, N, params, n_problems=n_problems, metric=metric,
                                seed=SEED, disturbance=base._disturbance(device, n_problems) if disturbed else None,
                                steps_per_graph=steps_per_graph, **kw)


@functools.lru_cache(maxsize=None)
def _reference(device, disturbed, step, max_iter=60):
    """The reference backend's 12 steps of the 6 problems, computed once per configuration."""
    loop = _batch(device, disturbed=disturbed, max_iter=max_iter)
    result = base._run(loop, base._x0(B), "reference", step)
    return result, base._bytes(result)


CONFIGS = {"plain": dict(disturbed=False, step=0), "disturbed": dict(disturbed=True, step=0),
           "past_the_end": dict(disturbed=True, step=33)}


def test_reference_backend_is_a_sound_yardstick(dev):
    """Valid info, and six distinct input logs: the replicates of a metric differ (their starts
    and draws do), and so do the metrics on the same replicate."""
    for c in CONFIGS.values():
        result, _ = _reference(dev, **c)
        base._check_result(result, n_problems=B)
        inputs = result[1]
        assert np.array_equal(result[0][:, 0].numpy(), base._x0(B))
        assert len({inputs[b].numpy().tobytes() for b in range(B)}) == B
    assert _batch(dev).metrics == METRICS


@pytest.mark.parametrize("backend,steps_per_graph", BACKENDS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_backends_equal_the_reference(dev, name, backend, steps_per_graph):
    c = CONFIGS[name]
    _, want = _reference(dev, **c)
    loop = _batch(dev, disturbed=c["disturbed"], steps_per_graph=steps_per_graph)
    result = base._run(loop, base._x0(B), backend, c["step"])
    base._check_result(result, n_problems=B)
    for what, g, w in zip(("states", "inputs", "info"), base._bytes(result), want):
        assert g == w, f"{name} {backend}/{steps_per_graph}: {what} differ"
    assert loop._state.cpu().tolist() == [[OFFSET + STEPS, c["step"] + STEPS]] * B


@pytest.mark.parametrize("backend,steps_per_graph", BACKENDS + [("reference", 1)])
def test_a_second_run_continues_the_first(dev, backend, steps_per_graph):
    """6 + 6 steps without a reset in between are the 12 steps."""
    whole, _ = _reference(dev, True, 0)
    loop = _batch(dev, disturbed=True, steps_per_graph=steps_per_graph)
    loop.reset(base._x0(B), step=0, stream_offset=OFFSET)
    first = tuple(t.cpu() for t in loop.run(6, backend=backend))
    second = tuple(t.cpu() for t in loop.run(6, backend=backend))
    joined = (torch.cat((first[0], second[0][:, 1:]), dim=1), torch.cat((first[1], second[1]), dim=1),
              torch.cat((first[2], second[2]), dim=1))
    assert base._bytes(joined) == base._bytes(whole)


@pytest.mark.parametrize("backend,steps_per_graph", [("graph", 3), ("launches", 1), ("reference", 1)])
@pytest.mark.parametrize("name", NAMES)
def test_equal_names_are_the_batch_with_that_string(dev, name, backend, steps_per_graph):
    """A sequence of B equal names: byte for byte the batch built with the string, with a
    RiskParams (the string batch's own draws: draw_period None) and with a RiskTable."""
    p = RiskParams(0.3, 0.3, 0.25, 0.05, 0.2)
    table = RiskTable(alpha=[0.2, 0.2, 0.2, 0.35, 0.35, 0.2], delta=0.1, epsilon=[0.05, 0.3, 0.15, 0.15, 0.05, 0.3])
    for params, period in ((p, None), (table, D)):
        kw = dict(draw_period=period) if isinstance(params, RiskTable) else {}
        plain = _batch(dev, metric=name, params=params, disturbed=True, steps_per_graph=steps_per_graph, **kw)
        assert plain.metrics == (name,) * B and plain.metric == name
        want = base._bytes(base._run(plain, base._x0(B), backend))
        loop = _batch(dev, metric=[name] * B, params=params, disturbed=True, steps_per_graph=steps_per_graph,
                      draw_period=period)
        assert loop.metrics == (name,) * B
        assert base._bytes(base._run(loop, base._x0(B), backend)) == want, type(params).__name__


@pytest.mark.parametrize("backend", ["reference", "graph", "launches"])
def test_common_random_numbers(dev, backend):
    """B = 3, draw_period = 1, equal starts, metrics (mean, cvar, dr_cvar): problem s's logs are
    byte for byte problem s of the B = 3 uniform batch of metric s with the same table and
    draw_period = 1 (the same data in the same position of the launch, the same solver workgroup
    size), and the three metrics give three different input logs."""
    table = RiskTable(alpha=0.2, delta=0.1, epsilon=[0.15, 0.15, 0.3])
    x0 = np.tile(base._start(), (3, 1))
    mixed = base._run(_batch(dev, metric=NAMES, params=table, draw_period=1, n_problems=3), x0, backend)
    base._check_result(mixed, n_problems=3)
    inputs = [mixed[1][s].numpy().tobytes() for s in range(3)]
    assert len(set(inputs)) == 3, "the constraints never bind: the scenario does not tell the metrics apart"
    for s, name in enumerate(NAMES):
        uniform = base._run(_batch(dev, metric=name, params=table, draw_period=1, n_problems=3), x0, backend)
        for got, want in zip(mixed, uniform):
            assert got[s].numpy().tobytes() == want[s].numpy().tobytes(), (backend, name)


def _evaluation():
    return LoopEvaluation(n_realizations=130, noise="laplace", noise_cov=np.diag([0.02, 0.08]),
                          robot_radius=0.3, obstacle_radius=0.3, seed=77, stream_offset=2 ** 32 - 2)


def test_the_evaluation_measures_the_metric_batch(dev):
    """With evaluate=, safety() of graph and launches equals the reference backend's for every
    tensor key, and the run is the run without an evaluation."""
    def run(backend, steps_per_graph=1):
        loop = _batch(dev, disturbed=True, steps_per_graph=steps_per_graph, evaluate=_evaluation())
        result = base._run(loop, base._x0(B), backend)
        return base._bytes(result), loop.safety()
    want_run, want = run("reference")
    assert want_run == _reference(dev, True, 0)[1]
    assert tuple(want["min_clearance"].shape) == (B, 130)
    for backend, steps_per_graph in BACKENDS:
        got_run, got = run(backend, steps_per_graph)
        assert got_run == want_run
        for k in TENSORS:
            assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), (backend, k)


def test_fallback_branches_side_by_side(dev):
    """A small interior-point cap, found at run time on the reference backend (the first of 1..8 at
    which the 12 x 6 statuses hold both solved and unsolved steps).  Solved and unsolved steps must
    both occur, and graph and launches must equal the reference at that cap."""
    found = None
    for cap in range(1, 9):
        result, want = _reference(dev, True, 0, max_iter=cap)
        solved = np.isin(result[2][..., _native.MPC_INFO_STATUS].numpy(), SOLVED)
        print(f"cap {cap}: solved steps per problem {solved.sum(axis=1).tolist()}")
        if solved.any() and (~solved).any():
            found = cap
            break
    assert found is not None, "no cap of 1..8 mixes solved and unsolved steps"
    base._check_result(result, n_problems=B)
    assert solved.any() and (~solved).any()
    for backend, steps_per_graph in BACKENDS:
        loop = _batch(dev, disturbed=True, steps_per_graph=steps_per_graph, max_iter=found)
        got = base._run(loop, base._x0(B), backend)
        base._check_result(got, n_problems=B)
        assert base._bytes(got) == want, (found, backend, steps_per_graph)
