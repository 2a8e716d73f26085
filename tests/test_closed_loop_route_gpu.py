"""GPU: a batch of receding-horizon loops with a reference path per problem
(simulation/closed_loop.py, RecedingHorizonBatch with ``x_ref_path [B, P, nx]`` and ``u_ref_path [B,
P, nu]``; the halfspace launch is drcvar_sampled_halfspaces_f64_route and the advance
drcvar_mpc_step_advance_batch_route_f64, include/drcvar_loop_route.h).

Setup: that of tests/test_closed_loop_batch_gpu.py, imported (main.py's multi_obstacle scenario,
H = 10, P = 40, N = 20, 12 steps from stream offset 2^32 - 4, B = 3, its starts) with three routes
from the scenario's start: to (4, 0) and to (4, 1) at 1.5, and to (3, -1) at 1.0.

Yardstick: the ``reference`` backend, which spells the route form out with what predates it: per
problem one engine.sampled_halfspaces call on that problem's own ego window, each problem's
METRIC_COLUMNS gathered with torch indexing, one filter_batch of all B problems, the advance in
torch ops with a per-problem index_select.  ``graph`` (1 and 3 steps per graph) and ``launches``
must give the same states, inputs and info (all ten columns) BIT FOR BIT.  No test here asserts
that a step is solved.
"""
import functools
import os

import numpy as np
import pytest
import torch

import test_closed_loop_batch_gpu as base
from conftest import GOLDEN_DIR
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.config.scenarios import get_scenario_config
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams, RiskTable
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.closed_loop import (
    LoopEvaluation, RecedingHorizonBatch, RecedingHorizonFilter)
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.planner import (
    ReferenceTrajectoryPlanner)

pytestmark = pytest.mark.gpu
STEPS, OFFSET, N, SEED, H, P, B = base.STEPS, base.OFFSET, base.N, base.SEED, base.H, base.P, base.B
BACKENDS, SOLVED = base.BACKENDS, base.SOLVED
GOALS = np.array([[4.0, 0.0], [4.0, 1.0], [3.0, -1.0]])
SPEEDS = np.array([1.5, 1.5, 1.0])
NAMES = ("mean", "cvar", "dr_cvar")
TABLE = RiskTable(alpha=[0.2, 0.35, 0.2], delta=0.1, epsilon=[0.05, 0.15, 0.3])
TENSORS = ("min_clearance", "collided", "step_hits", "step_collision_rate")
# what a loop filters with beside its route: a string with a RiskParams, names with a RiskTable
FORMS = {"dr_cvar": dict(metric="dr_cvar", params=None), "mixed": dict(metric=NAMES, params=TABLE)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _routes_host():
    """(x_ref [B, P, 4], u_ref [B, P, 2]) of the three routes, NumPy."""
    m = np.load(os.path.join(GOLDEN_DIR, "mpc_multi_obstacle_h30.npz"), allow_pickle=False)
    planner = ReferenceTrajectoryPlanner(m["A"], m["B"], m["C"], m["Q"], m["R"], P, base.DT)
    start = get_scenario_config("multi_obstacle")["ego_start"]
    x_ref, u_ref = planner.straight_line_routes(start, GOALS, SPEEDS)
    return np.ascontiguousarray(x_ref[:, :P]), np.ascontiguousarray(u_ref[:, :P]), tuple(m["p_bounds"])


def _routes(device, equal=False):
    x_ref, u_ref, _ = _routes_host()
    if equal:   # the shared path of the base setup, three times
        _, _, x2, u2 = base._setup(device)
        return x2[None].expand(B, -1, -1), u2[None].expand(B, -1, -1)
    return torch.from_numpy(x_ref).to(device), torch.from_numpy(u_ref).to(device)


def _batch(device, form="dr_cvar", disturbed=False, steps_per_graph=1, paths=None, **kw):
    model, nominal, _, _ = base._setup(device)
    x_ref, u_ref = _routes(device) if paths is None else paths
    f = FORMS[form]
    params = RiskParams() if f["params"] is None else f["params"]
    return RecedingHorizonBatch(model, nominal, x_ref, u_ref, N, params, n_problems=B, metric=f["metric"],
                                seed=SEED, disturbance=base._disturbance(device) if disturbed else None,
                                steps_per_graph=steps_per_graph, **kw)


@functools.lru_cache(maxsize=None)
def _reference(device, form, disturbed, step, max_iter=60):
    """The reference backend's 12 steps of the 3 problems, computed once per configuration."""
    loop = _batch(device, form, disturbed, max_iter=max_iter)
    result = base._run(loop, base._x0(), "reference", step)
    return result, base._bytes(result)


CONFIGS = {"plain": dict(disturbed=False, step=0), "disturbed": dict(disturbed=True, step=0),
           "past_the_end": dict(disturbed=True, step=33)}


def test_the_three_routes_are_what_the_docstring_says():
    """(needs no device) all inside the position box, the path ends, three distinct u_ref."""
    x_ref, u_ref, p_bounds = _routes_host()
    assert x_ref.shape == (B, P, 4) and u_ref.shape == (B, P, 2)
    lo, hi = np.asarray(p_bounds[0], dtype=float), np.asarray(p_bounds[1], dtype=float)
    assert np.all(x_ref[..., :2] >= lo) and np.all(x_ref[..., :2] <= hi)
    assert np.array_equal(x_ref[:, -1, :2], GOALS)
    start = get_scenario_config("multi_obstacle")["ego_start"]
    assert np.array_equal(x_ref[:, 0, :2], np.tile(start, (B, 1)))
    assert len({u_ref[b].tobytes() for b in range(B)}) == B
    assert 33 + H > P - 1


@pytest.mark.parametrize("form", list(FORMS))
def test_reference_backend_is_a_sound_yardstick(dev, form):
    """Valid info, the starts, and three distinct input logs."""
    for c in CONFIGS.values():
        result, _ = _reference(dev, form, **c)
        base._check_result(result)
        assert np.array_equal(result[0][:, 0].numpy(), base._x0())
        assert len({result[1][b].numpy().tobytes() for b in range(B)}) == B
    loop = _batch(dev, form)
    assert loop.routes and tuple(loop.ego_path.shape) == (B, P, 2)
    assert loop.x_ref_path.is_contiguous() and tuple(loop.u_ref_path.shape) == (B, P, 2)
    assert loop.metrics == (("dr_cvar",) * B if form == "dr_cvar" else NAMES) and loop.draw_period == B
    assert isinstance(loop.params, RiskTable) and len(loop.params) == B


@pytest.mark.parametrize("backend,steps_per_graph", BACKENDS)
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("form", list(FORMS))
def test_backends_equal_the_reference(dev, form, name, backend, steps_per_graph):
    c = CONFIGS[name]
    _, want = _reference(dev, form, **c)
    loop = _batch(dev, form, c["disturbed"], steps_per_graph)
    result = base._run(loop, base._x0(), backend, c["step"])
    base._check_result(result)
    for what, g, w in zip(("states", "inputs", "info"), base._bytes(result), want):
        assert g == w, f"{form} {name} {backend}/{steps_per_graph}: {what} differ"
    assert loop._state.cpu().tolist() == [[OFFSET + STEPS, c["step"] + STEPS]] * B


@pytest.mark.parametrize("backend,steps_per_graph", BACKENDS + [("reference", 1)])
def test_a_second_run_continues_the_first(dev, backend, steps_per_graph):
    """6 + 6 steps without a reset in between are the 12 steps."""
    whole, _ = _reference(dev, "mixed", True, 0)
    loop = _batch(dev, "mixed", True, steps_per_graph)
    loop.reset(base._x0(), step=0, stream_offset=OFFSET)
    first = tuple(t.cpu() for t in loop.run(6, backend=backend))
    second = tuple(t.cpu() for t in loop.run(6, backend=backend))
    joined = (torch.cat((first[0], second[0][:, 1:]), dim=1), torch.cat((first[1], second[1]), dim=1),
              torch.cat((first[2], second[2]), dim=1))
    assert base._bytes(joined) == base._bytes(whole)


@pytest.mark.parametrize("backend,steps_per_graph", [("graph", 3), ("launches", 1), ("reference", 1)])
@pytest.mark.parametrize("form", list(FORMS))
def test_equal_routes_are_the_batch_with_the_shared_path(dev, form, backend, steps_per_graph):
    """Three EQUAL 3-D routes: byte for byte the batch built with the 2-D path, and so is a batch
    with only one of the two paths given per problem."""
    model, nominal, x2, u2 = base._setup(dev)
    plain = _batch(dev, form, True, steps_per_graph, paths=(x2, u2))
    assert not plain.routes and plain.ego_path.dim() == 2
    want = base._bytes(base._run(plain, base._x0(), backend))
    x3, u3 = _routes(dev, equal=True)
    for paths in ((x3, u3), (x3, u2), (x2, u3.contiguous())):
        loop = _batch(dev, form, True, steps_per_graph, paths=paths)
        assert loop.routes and loop.x_ref_path.dim() == 3 and loop.u_ref_path.dim() == 3
        assert base._bytes(base._run(loop, base._x0(), backend)) == want, (form, backend)


@pytest.mark.parametrize("disturbed", [False, True])
def test_one_problem_is_the_single_loop(dev, disturbed):
    """B = 1 with [1, P, .] paths: RecedingHorizonFilter on that route, byte for byte, on the
    launches backend."""
    model, nominal, _, _ = base._setup(dev)
    x_ref, u_ref = _routes(dev)
    start = base._start()
    dist = base._disturbance(dev)[1] if disturbed else None
    for b in (1, 2):
        single = RecedingHorizonFilter(model, nominal, x_ref[b].contiguous(), u_ref[b].contiguous(), N,
                                       RiskParams(), seed=SEED, disturbance=dist)
        single.reset(start, stream_offset=OFFSET)
        want = tuple(t.cpu() for t in single.run(STEPS, backend="launches"))
        batch = RecedingHorizonBatch(model, nominal, x_ref[b:b + 1], u_ref[b:b + 1], N, RiskParams(),
                                     n_problems=1, seed=SEED,
                                     disturbance=None if dist is None else dist[None])
        got = base._run(batch, start, "launches")
        base._check_result(got, n_problems=1)
        assert base._bytes(tuple(t[0] for t in got)) == base._bytes(want), b


def test_the_predicted_form_with_distinct_routes(dev):
    """linearize="predicted", relinearize=1: step 1 stays the predicted-ego launch; the route
    advance and the priming follow each problem's own paths.  The backends equal its reference."""
    def run(backend, steps_per_graph=1):
        loop = _batch(dev, "dr_cvar", True, steps_per_graph, linearize="predicted", relinearize=1)
        assert loop.routes and loop._codes is None
        return base._run(loop, base._x0(), backend)
    want = run("reference")
    base._check_result(want)
    assert len({want[1][b].numpy().tobytes() for b in range(B)}) == B
    for backend, steps_per_graph in BACKENDS:
        assert base._bytes(run(backend, steps_per_graph)) == base._bytes(want), (backend, steps_per_graph)


def test_the_evaluation_measures_the_route_batch(dev):
    """With evaluate=, safety() of graph and launches equals the reference backend's for every
    tensor key, and the run is the run without an evaluation."""
    evaluation = LoopEvaluation(n_realizations=256, noise="laplace", noise_cov=np.diag([0.02, 0.08]),
                                robot_radius=0.3, obstacle_radius=0.3, seed=77, stream_offset=2 ** 32 - 2)

    def run(backend, steps_per_graph=1):
        loop = _batch(dev, "mixed", True, steps_per_graph, evaluate=evaluation)
        result = base._run(loop, base._x0(), backend)
        return base._bytes(result), loop.safety()
    want_run, want = run("reference")
    assert want_run == _reference(dev, "mixed", True, 0)[1]
    assert tuple(want["min_clearance"].shape) == (B, 256)
    for backend, steps_per_graph in BACKENDS:
        got_run, got = run(backend, steps_per_graph)
        assert got_run == want_run
        for k in TENSORS:
            assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), (backend, k)


def _compare_at_cap(dev, cap):
    result, want = _reference(dev, "dr_cvar", True, 0, max_iter=cap)
    base._check_result(result)
    for backend, steps_per_graph in BACKENDS:
        loop = _batch(dev, "dr_cvar", True, steps_per_graph, max_iter=cap)
        got = base._run(loop, base._x0(), backend)
        base._check_result(got)
        assert base._bytes(got) == want, (cap, backend, steps_per_graph)
    return np.isin(result[2][..., _native.MPC_INFO_STATUS].numpy(), SOLVED)


def test_a_small_iteration_cap(dev):
    """max_iter = 3, the 2-D batch's first mix of solved and unsolved steps for dr_cvar: the
    backends agree bit for bit whatever the statuses are.  Whether both kinds occur is read from
    the reference backend's own info: if they do not at 3, the cap is walked upward (4..8) to the
    first at which they do, that cap is printed, and the backends are compared there too; nothing
    is asserted about which steps are solved."""
    solved = _compare_at_cap(dev, 3)
    print(f"cap 3: solved steps per problem {solved.sum(axis=1).tolist()}")
    if solved.any() and (~solved).any():
        return
    for cap in range(4, 9):
        result, _ = _reference(dev, "dr_cvar", True, 0, max_iter=cap)
        solved = np.isin(result[2][..., _native.MPC_INFO_STATUS].numpy(), SOLVED)
        print(f"cap {cap}: solved steps per problem {solved.sum(axis=1).tolist()}")
        if solved.any() and (~solved).any():
            mixed = _compare_at_cap(dev, cap)
            assert mixed.any() and (~mixed).any()
            print(f"the first cap that mixes solved and unsolved steps: {cap}")
            return
    print("no cap of 3..8 mixes solved and unsolved steps on these routes")


def test_wrong_route_shapes(dev):
    model, nominal, x2, u2 = base._setup(dev)
    x3, u3 = _routes(dev)
    for x_ref, u_ref in ((x3[:2], u3), (x3, u3[:2]), (x3[:, :P - 1], u3), (x2, u3[:1])):
        with pytest.raises(ValueError):
            RecedingHorizonBatch(model, nominal, x_ref, u_ref, N, RiskParams(), n_problems=B)
