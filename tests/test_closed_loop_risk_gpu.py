"""GPU: a batch of receding-horizon loops with risk parameters per problem and shared draws
(simulation/closed_loop.py, RecedingHorizonBatch(params=RiskTable(...), draw_period=D); the
halfspace launch is drcvar_sampled_halfspaces_f64_risk, include/drcvar_loop_risk.h).

Setup: that of tests/test_closed_loop_batch_gpu.py, imported (main.py's multi_obstacle scenario,
H = 10, P = 40, N = 20, 12 steps from stream offset 2^32 - 4) with B = 6 problems: 3 settings of
(alpha, delta, epsilon) x D = 2 replicates, problem b = s D + r, every problem with a start of its
own.

Yardstick: the ``reference`` backend, which spells the table form out with the entry that predates
it — per problem one engine.sampled_halfspaces call with ``params.row(b)`` on the unit window of
draw problem ``b mod D``, then one filter_batch of all B problems.  ``graph`` (1 and 3 steps per
graph) and ``launches`` must give the same states, inputs and info — all ten columns — BIT FOR BIT.
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
S, D = 3, 2
B = S * D
SETTINGS = ((0.2, 0.1, 0.05), (0.2, 0.1, 0.3), (0.35, 0.05, 0.15))     # (alpha, delta, epsilon)
TENSORS = ("min_clearance", "collided", "step_hits", "step_collision_rate")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _table(settings=SETTINGS, replicates=D):
    rows = [s for s in settings for _ in range(replicates)]           # b = s D + r
    return RiskTable(alpha=[r[0] for r in rows], delta=[r[1] for r in rows], epsilon=[r[2] for r in rows])


def _batch(device, params=None, draw_period=D, disturbed=False, steps_per_graph=1, n_problems=B, **kw):
    model, nominal, x_ref, u_ref = base._setup(device)
    params = _table() if params is None else params
    if isinstance(params, RiskTable):
        kw["draw_period"] = draw_period
    return RecedingHorizonBatch(model, nominal, x_ref, u_ref, N, params, n_problems=n_problems, seed=SEED,
                                disturbance=base._disturbance(device, n_problems) if disturbed else None,
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
    """Valid info; the replicates of a setting differ (their starts and draws do), and so do the
    settings on the same replicate (their rows do)."""
    for c in CONFIGS.values():
        result, _ = _reference(dev, **c)
        base._check_result(result, n_problems=B)
        inputs = result[1]
        assert np.array_equal(result[0][:, 0].numpy(), base._x0(B))
        assert len({inputs[b].numpy().tobytes() for b in range(B)}) == B


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
    """6 + 6 steps without a reset in between are the 12 steps, twice over."""
    whole, _ = _reference(dev, True, 0)
    loop = _batch(dev, disturbed=True, steps_per_graph=steps_per_graph)
    for _ in range(2):
        loop.reset(base._x0(B), step=0, stream_offset=OFFSET)
        first = tuple(t.cpu() for t in loop.run(6, backend=backend))
        second = tuple(t.cpu() for t in loop.run(6, backend=backend))
        joined = (torch.cat((first[0], second[0][:, 1:]), dim=1), torch.cat((first[1], second[1]), dim=1),
                  torch.cat((first[2], second[2]), dim=1))
        assert base._bytes(joined) == base._bytes(whole)


@pytest.mark.parametrize("backend,steps_per_graph", [("graph", 3), ("launches", 1), ("reference", 1)])
def test_equal_rows_are_the_batch_with_those_scalars(dev, backend, steps_per_graph):
    """A table of B equal rows with draw_period=None: the batch built with the matching RiskParams,
    byte for byte."""
    p = RiskParams(0.3, 0.3, 0.25, 0.05, 0.2)
    plain = _batch(dev, params=p, disturbed=True, steps_per_graph=steps_per_graph)
    want = base._bytes(base._run(plain, base._x0(B), backend))
    table = RiskTable(alpha=[p.alpha] * B, delta=p.delta, epsilon=p.epsilon)
    loop = _batch(dev, params=table, draw_period=None, disturbed=True, steps_per_graph=steps_per_graph)
    assert loop.draw_period == B
    assert base._bytes(base._run(loop, base._x0(B), backend)) == want


@pytest.mark.parametrize("backend", ["graph", "reference"])
def test_one_draw_period_is_common_random_numbers(dev, backend):
    """D = 1, equal starts: problems 0 and 2 have equal rows and give the same logs, byte for byte;
    problem 1 differs from them in epsilon alone and gives others."""
    table = RiskTable(alpha=0.2, delta=0.1, epsilon=[0.15, 0.6, 0.15])
    loop = _batch(dev, params=table, draw_period=1, n_problems=3)
    result = base._run(loop, base._start(), backend)
    base._check_result(result, n_problems=3)
    for t in result:
        assert t[0].numpy().tobytes() == t[2].numpy().tobytes()
    assert result[1][0].numpy().tobytes() != result[1][1].numpy().tobytes()
    # with a period of its own every problem draws for itself: 0 and 2 part
    own = base._run(_batch(dev, params=table, draw_period=3, n_problems=3), base._start(), backend)
    assert own[1][0].numpy().tobytes() == result[1][0].numpy().tobytes()
    assert own[1][2].numpy().tobytes() != result[1][2].numpy().tobytes()


def _evaluation():
    return LoopEvaluation(n_realizations=130, noise="laplace", noise_cov=np.diag([0.02, 0.08]),
                          robot_radius=0.3, obstacle_radius=0.3, seed=77, stream_offset=2 ** 32 - 2)


def test_the_evaluation_measures_the_table_batch(dev):
    """With evaluate=, safety() of graph and launches equals the reference backend's, and the run
    is the run without an evaluation."""
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
        assert got["metrics"] == want["metrics"]


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
