"""GPU: a batch of receding-horizon loops with a noise factor per obstacle and look-ahead step
(simulation/closed_loop.py, RecedingHorizonBatch with ``noise=engine.NoiseTable``; the halfspace
launch is drcvar_sampled_halfspaces_f64_noise, include/drcvar_loop_noise.h).

Setup: that of tests/test_closed_loop_batch_gpu.py, imported (main.py's multi_obstacle scenario,
H = 10, P = 40, N = 20, 12 steps from stream offset 2^32 - 4, B = 3, its starts), the routes of
tests/test_closed_loop_route_gpu.py where a route per problem is asked for.  The schedule is
``scaled(DEFAULT_NOISE_COV, 1 + 0.5 t)``, made per problem by a further factor of (1, 2, 4).

Yardstick: the ``reference`` backend, which spells the noise form out with what predates it: per
problem and distinct factor one engine.sampled_halfspaces call with ``chol=f``, from which the units
that carry ``f`` are taken.  ``graph`` (1 and 3 steps per graph) and ``launches`` must give the same
states, inputs and info BIT FOR BIT.  No test here asserts that a step is solved.
"""
import functools

import numpy as np
import pytest
import torch

import test_closed_loop_batch_gpu as base
import test_closed_loop_route_gpu as route
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import (
    DEFAULT_NOISE_COV, NoiseTable, RiskParams, RiskTable)
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.closed_loop import (
    LoopEvaluation, RecedingHorizonBatch)

pytestmark = pytest.mark.gpu
STEPS, OFFSET, N, SEED, H, P, B = base.STEPS, base.OFFSET, base.N, base.SEED, base.H, base.P, base.B
BACKENDS = base.BACKENDS
NAMES, TABLE, TENSORS = route.NAMES, route.TABLE, route.TENSORS
GROWTH = 1.0 + 0.5 * np.arange(H)
PER_PROBLEM = (1.0, 2.0, 4.0)
FORMS = {"dr_cvar": dict(metric="dr_cvar", params=None), "mixed": dict(metric=NAMES, params=None),
         "risk_table": dict(metric=NAMES, params=TABLE, draw_period=1)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _schedule(n_obstacles, per_problem=PER_PROBLEM):
    scales = np.asarray(per_problem)[:, None, None] * np.broadcast_to(GROWTH, (B, n_obstacles, H))
    return NoiseTable.scaled(DEFAULT_NOISE_COV, scales)


def _batch(device, form="dr_cvar", steps_per_graph=1, routes=False, noise="schedule", **kw):
    model, nominal, x_ref, u_ref = base._setup(device)
    if routes:
        x_ref, u_ref = route._routes(device)
    f = dict(FORMS[form])
    params = f.pop("params") or RiskParams()
    if noise == "schedule":
        noise = _schedule(nominal.shape[-3])
    return RecedingHorizonBatch(model, nominal, x_ref, u_ref, N, params, n_problems=B, seed=SEED,
                                disturbance=base._disturbance(device), steps_per_graph=steps_per_graph,
                                noise=noise, **f, **kw)


@functools.lru_cache(maxsize=None)
def _reference(device, form, routes):
    loop = _batch(device, form, routes=routes)
    result = base._run(loop, base._x0(), "reference")
    return result, base._bytes(result)


CASES = [("dr_cvar", False), ("mixed", False), ("risk_table", False), ("mixed", True)]


@pytest.mark.parametrize("form,routes", CASES)
def test_reference_backend_is_a_sound_yardstick(dev, form, routes):
    result, _ = _reference(dev, form, routes)
    base._check_result(result)
    assert np.array_equal(result[0][:, 0].numpy(), base._x0())
    loop = _batch(dev, form, routes=routes)
    assert loop.routes == routes and loop.ego_path.dim() == (3 if routes else 2)
    assert loop._noise_period == B * loop.n_obstacles
    assert isinstance(loop.params, RiskTable) and len(loop.params) == B and len(loop.metrics) == B
    # the schedule grows along the horizon and differs between the problems
    assert len({loop.noise.factor(0, t) for t in range(H)}) == H
    assert len({loop.noise.factor(b * loop.n_obstacles, 0) for b in range(B)}) == B


@pytest.mark.parametrize("backend,steps_per_graph", BACKENDS)
@pytest.mark.parametrize("form,routes", CASES)
def test_backends_equal_the_reference(dev, form, routes, backend, steps_per_graph):
    _, want = _reference(dev, form, routes)
    loop = _batch(dev, form, steps_per_graph, routes=routes)
    result = base._run(loop, base._x0(), backend)
    base._check_result(result)
    for what, g, w in zip(("states", "inputs", "info"), base._bytes(result), want):
        assert g == w, f"{form} routes={routes} {backend}/{steps_per_graph}: {what} differ"
    assert loop._state.cpu().tolist() == [[OFFSET + STEPS, STEPS]] * B


def test_the_evaluation_measures_the_noise_batch(dev):
    evaluation = LoopEvaluation(n_realizations=256, noise="laplace", noise_cov=np.diag([0.02, 0.08]),
                                robot_radius=0.3, obstacle_radius=0.3, seed=77, stream_offset=2 ** 32 - 2)

    def run(backend, steps_per_graph=1):
        loop = _batch(dev, "mixed", steps_per_graph, evaluate=evaluation)
        result = base._run(loop, base._x0(), backend)
        return base._bytes(result), loop.safety()
    want_run, want = run("reference")
    assert want_run == _reference(dev, "mixed", False)[1]
    for backend, steps_per_graph in BACKENDS:
        got_run, got = run(backend, steps_per_graph)
        assert got_run == want_run
        for k in TENSORS:
            assert got[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), (backend, k)


@pytest.mark.parametrize("backend,steps_per_graph", [("graph", 3), ("launches", 1), ("reference", 1)])
@pytest.mark.parametrize("form", ["dr_cvar", "mixed"])
def test_the_constant_schedule_is_the_batch_without_noise(dev, form, backend, steps_per_graph):
    plain = _batch(dev, form, steps_per_graph, noise=None)
    assert plain.noise is None and plain._noise_rows is None
    want = base._bytes(base._run(plain, base._x0(), backend))
    for shape in ((H,), (plain.n_obstacles, H), (B, plain.n_obstacles, H)):
        loop = _batch(dev, form, steps_per_graph, noise=NoiseTable.scaled(DEFAULT_NOISE_COV, np.ones(shape)))
        assert base._bytes(base._run(loop, base._x0(), backend)) == want, (form, backend, shape)


def test_a_schedule_changes_its_own_problem_only(dev):
    def run(per_problem):
        model, nominal, _, _ = base._setup(dev)
        loop = _batch(dev, "dr_cvar", 3, noise=_schedule(nominal.shape[-3], per_problem))
        return base._run(loop, base._x0(), "graph")
    a, b = run(PER_PROBLEM), run((1.0, 3.0, 4.0))
    for x, y in zip(a, b):
        for p in (0, 2):
            assert x[p].numpy().tobytes() == y[p].numpy().tobytes()
    assert a[1][1].numpy().tobytes() != b[1][1].numpy().tobytes()
