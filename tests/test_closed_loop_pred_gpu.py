"""GPU: the receding-horizon loops linearised about their own predicted path
(simulation/closed_loop.py, linearize="predicted", relinearize=r; the halfspace launch is
drcvar_sampled_halfspaces_f64_pred on the loop's x0 and the solver's x_out).

Setup: that of tests/test_closed_loop_batch_gpu.py, imported (main.py's multi_obstacle scenario,
H = 10, P = 40, N = 20, B = 3 with its X0_OFFSETS, 12 steps from stream offset 2^32 - 4).

Yardstick: the ``reference`` backend, which spells the predicted form out with entries that
predate it — per problem the ego by a torch multiply-and-add chain over the states and
engine.sampled_halfspaces on the problem's unit window, then one filter_batch of all B problems.
The model's C selects the two positions, so every product of the chain is exact and it rounds
where the kernel's fma chain rounds: ``graph`` (1 and 3 steps per graph) and ``launches`` must
give the same states, inputs and info — all ten columns — BIT FOR BIT.
"""
import functools

import numpy as np
import pytest
import torch

import test_closed_loop_batch_gpu as base
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.closed_loop import (
    LoopEvaluation, RecedingHorizonFilter)

pytestmark = pytest.mark.gpu
B, STEPS, OFFSET, N, SEED, H = base.B, base.STEPS, base.OFFSET, base.N, base.SEED, base.H
BACKENDS = base.BACKENDS
SOLVED = base.SOLVED
TENSORS = ("min_clearance", "collided", "step_hits", "step_collision_rate")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _batch(device, metric="dr_cvar", disturbed=False, steps_per_graph=1, relinearize=0,
           linearize="predicted", **kw):
    return base._batch(device, metric, base._disturbance(device) if disturbed else None, steps_per_graph,
                       linearize=linearize, relinearize=relinearize, **kw)


@functools.lru_cache(maxsize=None)
def _reference(device, metric, disturbed, step, relinearize, max_iter=60):
    """The reference backend's 12 steps of the 3 problems, computed once per configuration."""
    loop = _batch(device, metric, disturbed, relinearize=relinearize, max_iter=max_iter)
    result = base._run(loop, base._x0(), "reference", step)
    trace = [tuple(t.cpu() for t in row) for row in loop.reference_trace]
    return result, base._bytes(result), trace


CONFIGS = {
    "dr_cvar": dict(metric="dr_cvar", disturbed=False, step=0, relinearize=0),
    "mean_disturbed": dict(metric="mean", disturbed=True, step=0, relinearize=0),
    "dr_cvar_disturbed": dict(metric="dr_cvar", disturbed=True, step=0, relinearize=0),
    "mean": dict(metric="mean", disturbed=False, step=0, relinearize=0),
    "past_the_end": dict(metric="dr_cvar", disturbed=True, step=33, relinearize=0),
    "dr_cvar_relinearized": dict(metric="dr_cvar", disturbed=True, step=0, relinearize=1),
    "mean_relinearized": dict(metric="mean", disturbed=False, step=0, relinearize=1),
    "past_the_end_relinearized": dict(metric="dr_cvar", disturbed=True, step=33, relinearize=1),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_reference_backend_is_a_sound_yardstick(dev, name):
    """Valid info; states[b, i + 1] is row 1 of step i's LAST solve of problem b (+ its disturbance
    row); the problems differ, and the run differs from the loop linearised about the reference."""
    c = CONFIGS[name]
    result, got, trace = _reference(dev, **c)
    base._check_result(result)
    states, inputs, info = result
    disturbance = base._disturbance("cpu")
    assert np.array_equal(states[:, 0].numpy(), base._x0()) and len(trace) == STEPS
    for i, (x, u, inf) in enumerate(trace):
        want = x[:, 1] + disturbance[:, i] if c["disturbed"] else x[:, 1]
        assert torch.equal(states[:, i + 1], want), i
        assert torch.equal(inputs[:, i], u[:, 0])
        assert inf.numpy().tobytes() == info[:, i].contiguous().numpy().tobytes()
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not torch.equal(inputs[a], inputs[b])
    # the mean halfspace (columns 0..2 of a record) is taken about the origin, not the ego: under
    # metric="mean" the linearisation point cannot matter, under dr_cvar it must
    _, plain, _ = base._reference(dev, c["metric"], c["disturbed"], c["step"])
    assert (got[1] == plain[1]) == (c["metric"] == "mean")
    if c["relinearize"]:
        once = _reference(dev, c["metric"], c["disturbed"], c["step"], 0)[1]
        assert (got[1] == once[1]) == (c["metric"] == "mean")


@pytest.mark.parametrize("backend,steps_per_graph", BACKENDS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_backends_equal_the_reference(dev, name, backend, steps_per_graph):
    c = CONFIGS[name]
    _, want, _ = _reference(dev, **c)
    loop = _batch(dev, c["metric"], c["disturbed"], steps_per_graph, c["relinearize"])
    result = base._run(loop, base._x0(), backend, c["step"])
    base._check_result(result)
    for what, g, w in zip(("states", "inputs", "info"), base._bytes(result), want):
        assert g == w, f"{name} {backend}/{steps_per_graph}: {what} differ"
    assert loop._state.cpu().tolist() == [[OFFSET + STEPS, c["step"] + STEPS]] * B


@pytest.mark.parametrize("relinearize", [0, 1])
@pytest.mark.parametrize("backend,steps_per_graph", BACKENDS + [("reference", 1)])
def test_a_second_run_continues_the_first(dev, backend, steps_per_graph, relinearize):
    """6 + 6 steps without a reset in between are the 12 steps, and a second reset gives the same
    bytes again (the eager step before the capture left no trace in x_out)."""
    whole, _, _ = _reference(dev, "dr_cvar", True, 0, relinearize)
    loop = _batch(dev, "dr_cvar", True, steps_per_graph, relinearize)
    for _ in range(2):
        loop.reset(base._x0(), step=0, stream_offset=OFFSET)
        first = tuple(t.cpu() for t in loop.run(6, backend=backend))
        second = tuple(t.cpu() for t in loop.run(6, backend=backend))
        joined = (torch.cat((first[0], second[0][:, 1:]), dim=1), torch.cat((first[1], second[1]), dim=1),
                  torch.cat((first[2], second[2]), dim=1))
        assert base._bytes(joined) == base._bytes(whole)


@pytest.mark.parametrize("relinearize", [0, 1])
@pytest.mark.parametrize("disturbed", [False, True])
def test_one_problem_is_the_single_loop(dev, disturbed, relinearize):
    """B = 1: the batch and RecedingHorizonFilter, byte for byte, on the graph backend; and the
    single class's graph against its own reference backend."""
    model, nominal, x_ref, u_ref = base._setup(dev)
    start = base._start() + base.X0_OFFSETS[1]
    dist = base._disturbance(dev)[1] if disturbed else None
    single = RecedingHorizonFilter(model, nominal, x_ref, u_ref, N, RiskParams(), seed=SEED, disturbance=dist,
                                   linearize="predicted", relinearize=relinearize)
    single.reset(start, stream_offset=OFFSET)
    want = tuple(t.cpu() for t in single.run(STEPS, backend="graph"))
    single.reset(start, stream_offset=OFFSET)
    assert base._bytes(tuple(t.cpu() for t in single.run(STEPS, backend="reference"))) == base._bytes(want)
    batch = base._batch(dev, disturbance=None if dist is None else dist[None], n_problems=1,
                        linearize="predicted", relinearize=relinearize)
    got = base._run(batch, start, "graph")
    base._check_result(got, n_problems=1)
    assert base._bytes(tuple(t[0] for t in got)) == base._bytes(want)


@pytest.mark.parametrize("relinearize", [0, 1])
def test_fallback_branches_side_by_side(dev, relinearize):
    """A small interior-point cap, found at run time on the reference backend (the first of 1..8 at
    which the 12 x 3 statuses hold both solved and unsolved steps): after an unsolved step x_out is
    the rolled-out fallback, and the next step linearises about it.  Solved and unsolved steps must
    both occur, and graph and launches must equal the reference at that cap."""
    found = None
    for cap in range(1, 9):
        result, want, _ = _reference(dev, "dr_cvar", True, 0, relinearize, max_iter=cap)
        solved = np.isin(result[2][..., _native.MPC_INFO_STATUS].numpy(), SOLVED)
        print(f"cap {cap}: solved steps per problem {solved.sum(axis=1).tolist()}")
        if solved.any() and (~solved).any():
            found = cap
            break
    assert found is not None, "no cap of 1..8 mixes solved and unsolved steps"
    base._check_result(result)
    assert solved.any() and (~solved).any()
    for backend, steps_per_graph in BACKENDS:
        loop = _batch(dev, "dr_cvar", True, steps_per_graph, relinearize, max_iter=found)
        got = base._run(loop, base._x0(), backend)
        base._check_result(got)
        assert base._bytes(got) == want, (found, backend, steps_per_graph)


def _evaluation():
    return LoopEvaluation(n_realizations=130, noise="laplace", noise_cov=np.diag([0.02, 0.08]),
                          robot_radius=0.3, obstacle_radius=0.3, seed=77, stream_offset=2 ** 32 - 2)


@pytest.mark.parametrize("relinearize", [0, 1])
def test_the_evaluation_measures_the_predicted_loop(dev, relinearize):
    """With evaluate=, safety() of graph and launches equals the reference backend's, and the run
    is the run without an evaluation."""
    def run(backend, steps_per_graph=1):
        loop = _batch(dev, "dr_cvar", True, steps_per_graph, relinearize, evaluate=_evaluation())
        result = base._run(loop, base._x0(), backend)
        return base._bytes(result), loop.safety()
    want_run, want = run("reference")
    assert want_run == _reference(dev, "dr_cvar", True, 0, relinearize)[1]
    for backend, steps_per_graph in BACKENDS:
        got_run, got = run(backend, steps_per_graph)
        assert got_run == want_run
        for k in TENSORS:
            assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), (backend, k)
        assert got["metrics"] == want["metrics"]


@pytest.mark.parametrize("backend,steps_per_graph", BACKENDS + [("reference", 1)])
def test_explicit_reference_linearisation_is_the_default(dev, backend, steps_per_graph):
    want = base._reference(dev, "dr_cvar", True, 0)[1]
    loop = _batch(dev, "dr_cvar", True, steps_per_graph, linearize="reference")
    assert base._bytes(base._run(loop, base._x0(), backend)) == want


@pytest.mark.parametrize("backend", ["graph", "reference"])
def test_the_first_step_sees_each_problems_own_start(dev, backend):
    """After reset the prediction is the reference path, so the first step differs from the default
    class's exactly through x0: problem 0 starts on the reference path (offset zero) and its first
    logged row is byte-equal; problems 1 and 2 start off it and theirs differ."""
    plain = base._run(base._batch(dev), base._x0(), backend, steps=3 if backend == "graph" else 1)
    got = base._run(_batch(dev, steps_per_graph=3 if backend == "graph" else 1), base._x0(), backend,
                    steps=3 if backend == "graph" else 1)
    for t_plain, t_got in zip(plain[1:], got[1:]):                    # inputs and info, step 0
        assert t_got[0, 0].numpy().tobytes() == t_plain[0, 0].numpy().tobytes()
        for b in (1, 2):
            assert t_got[b, 0].numpy().tobytes() != t_plain[b, 0].numpy().tobytes(), b
    assert torch.equal(got[0][0, 1], plain[0][0, 1])
    assert not torch.equal(got[0][1, 1], plain[0][1, 1]) and not torch.equal(got[0][2, 1], plain[0][2, 1])


def test_130_problems(dev):
    """B = 130 crosses the solver's 128-problem workgroup-size rule: 4 steps, graph against
    reference, every problem with its own start and disturbance, one relinearisation."""
    n, steps = 130, 4
    x0, dist = base._x0(n), base._disturbance(dev, n)
    kw = dict(disturbance=dist, n_problems=n, linearize="predicted", relinearize=1)
    want = base._run(base._batch(dev, **kw), x0, "reference", steps=steps)
    got = base._run(base._batch(dev, steps_per_graph=2, **kw), x0, "graph", steps=steps)
    base._check_result(got, n_problems=n, steps=steps)
    assert base._bytes(got) == base._bytes(want)
    assert len({got[1][b].numpy().tobytes() for b in range(n)}) == n   # the problems are distinct


def test_a_step_is_three_plus_two_r_launches(dev):
    """The captured step: halfspaces, solve, r x (halfspaces, solve), advance (+ the evaluation)."""
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import engine
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import closed_loop
    counts = {}
    for r, evaluate in ((0, None), (1, None), (2, None), (1, _evaluation())):
        loop = _batch(dev, relinearize=r, evaluate=evaluate)
        loop.reset(base._x0(), stream_offset=OFFSET)
        step = loop._make_step(torch.cuda.current_stream(dev))
        calls = []
        launch, solve = engine.PreparedLaunch.__call__, closed_loop.filter_batch
        try:
            engine.PreparedLaunch.__call__ = lambda self: (calls.append("launch"), launch(self))[1]
            closed_loop.filter_batch = lambda *a, **k: (calls.append("solve"), solve(*a, **k))[1]
            step()
        finally:
            engine.PreparedLaunch.__call__, closed_loop.filter_batch = launch, solve
        counts[(r, evaluate is not None)] = len(calls)
        assert calls[:2] == ["launch", "solve"] and calls.count("solve") == 1 + r
    torch.cuda.synchronize()
    assert counts == {(0, False): 3, (1, False): 5, (2, False): 7, (1, True): 6}
