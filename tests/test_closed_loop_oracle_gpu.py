"""GPU: every logged step of the receding-horizon loops (simulation/closed_loop.py) held to the
all-host oracle of tests/closed_loop_oracle.py: Philox mirror -> long-double halfspace reference ->
KKT-certified QP, none of which runs a line of the engine.

The other closed-loop modules compare the ``graph`` and ``launches`` backends bit for bit with the
``reference`` backend, which runs the same halfspace and QP kernels on windows gathered by torch
ops: a wiring mistake both sides share (the offset of step i, the rows of a clamped window, the
draw unit, the noise row, whose route, metric or risk row a problem reads, the fallback memory)
passes them.  Here the ``reference`` backend runs once (its logs and ``reference_trace``, the
device's full x, u and info of every step), ``graph`` with 3 steps per graph must give the same
bytes, and every step of every problem is then rebuilt on the host FROM THE STATE THE DEVICE LOGGED
FOR IT (bitwise; so solver tolerance never compounds) and compared:

* solved steps: trace u and x over the whole horizon against the oracle's, MPC_TOL where the
  device polished and UNPOLISHED_TOL otherwise; polished steps also objective (1e-6 relative) and
  largest slack (1e-6), as tests/test_mpc.py does; the oracle's own answer must be ``optimal`` with
  every KKT residual below 1e-8;
* unsolved steps (capped runs): USED_FALLBACK, trace u bitwise ``mpc_qp.fallback_inputs`` of the
  device's own memory, trace x its rollout within 1e-12.  The memory is the trace u of the last
  solved step (none: the ``u_ref`` window is rolled out); it stays as it is while steps fail, so
  every failed step rolls out that u shifted by one row with the window's last ``u_ref`` row at
  the tail (include/drcvar_mpc.h, steps 3 and 6; the reference's ``_fallback`` never stores what
  it returns);
* from the answer alone: x[0] bitwise the logged state, x[1:] the long-double rollout of u within
  the ``roll_tol`` of tests/test_mpc_bounds_gpu.py, and on solved steps u and C x inside their
  boxes to MPC_TOL.  An unsolved step's answer is the fallback inputs rolled out, which no box
  binds (the reference's ``_fallback`` has none): the straight-line ``u_ref`` starts from rest with
  an input of 7.47 against the box's 5, which S3_cap3's step 0 rolls out, and S3_mean's step 9
  coasts to x = 10.12 against 10;
* the advance: inputs[i] bitwise u[0], info[i] the trace's bytes, states[i + 1] bitwise x[1] plus
  the disturbance row;
* the halfspace record, directly (the QP sees only active rows): after graph runs of 1, 5 and 12
  steps the loop's record buffer (and the batch's selected buffer) against the host record of the
  last step run, every column of every unit, within ``closed_loop_oracle.record_tolerance``; the
  status words, from the same entry launched once more on the last step's state with a status
  buffer (its record must be the loop's, bit for bit), must be UNIT_OK.

Cases: S1 single loop, N = 200, dr_cvar and mean, disturbed, from step 0; S2 single, dr_cvar from
step 33 (every window clamped at the path's end); S3 the capped runs MIXED_CAPS of
tests/test_closed_loop_gpu.py (both fallback branches); B1 batch of 3, N = 20, RiskParams, one
metric, independent draws; B2 batch of 3 with routes, RiskTable, a metric per problem and the noise
schedule, draw period 1 and 3 (None).  H = 10, P = 40, 12 steps from stream offset 2^32 - 4.
S1, S2, B1 and B2 require every step solved.

Out of scope here: ``linearize="predicted"`` / ``relinearize`` (the linearisation point is the
previous step's whole predicted path: the follow-up), ``LoopEvaluation`` and clustered solves.

Measured on an MI355X (docs/lab_notebook.md §5b); every solved step came back polished:

    case            solved   largest |u - u_oracle|   largest record error / tolerance
    S1_dr_cvar      12 / 12  2.8e-10                  0.009
    S1_mean         12 / 12  2.9e-10                  (S1_dr_cvar's draws)
    S2              12 / 12  5.2e-12                  0.016
    S3_cap3          3 / 12  5.2e-15 (9 unsolved steps roll out u_ref, then 3 solved)
    S3_cap4          5 / 12  2.8e-10 (7 unsolved steps roll out step 0's optimum, shifted)
    S3_mean          1 / 12  1.4e-10 (11 unsolved steps roll out step 0's optimum, shifted)
    B1              36 / 36  1.3e-10                  0.033
    B2_period1      36 / 36  2.5e-10                  0.032
    B2_independent  36 / 36  2.5e-10                  0.033

The record tolerances themselves are 1e-13 to 2e-12 (tests/test_closed_loop_oracle_host.py).  With
the stream offset frozen, the next problem's route or the next problem's metric planted in the
``reference`` backend's step, the step tests of every case the mistake can reach fail at the
comparison of u with the oracle's (offset: all nine; route and metric: both B2 cases).
"""
import functools
import os

import numpy as np
import pytest
import torch

import closed_loop_oracle as clo
import test_closed_loop_batch_gpu as base
import test_closed_loop_gpu as single
import test_closed_loop_noise_gpu as noise
import test_closed_loop_route_gpu as route
from conftest import GOLDEN_DIR, OFFSET_TOL
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import (
    DEFAULT_NOISE_COV, NoiseTable, RiskParams)
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.closed_loop import (
    RecedingHorizonBatch)
from oracle import mpc_qp
from test_mpc import MPC_TOL
from test_mpc_bounds_gpu import UNPOLISHED_TOL

pytestmark = pytest.mark.gpu
H, P, STEPS, OFFSET, B = single.H, single.P, single.STEPS, single.OFFSET, base.B
assert (H, P, STEPS, OFFSET) == (10, 40, 12, 2 ** 32 - 4) == (base.H, base.P, base.STEPS, base.OFFSET)
SOLVED = single.SOLVED
MODEL = clo.load_model(os.path.join(GOLDEN_DIR, "mpc_multi_obstacle_h30.npz"))
CHOL = NoiseTable.scaled(DEFAULT_NOISE_COV, np.ones(H)).factor(0, 0)   # the factor of DEFAULT_NOISE_COV
RECORD_RUNS = (1, 5, 12)

SINGLE_CASES = {"S1_dr_cvar": "dr_cvar_disturbed", "S1_mean": "mean_disturbed", "S2": "past_the_end",
                "S3_cap3": "mix_cap3", "S3_cap4": "mix_cap4", "S3_mean": "mix_mean"}
BATCH_CASES = {"B1": None, "B2_period1": 1, "B2_independent": None}
ALL_SOLVED = ("S1_dr_cvar", "S1_mean", "S2", "B1", "B2_period1", "B2_independent")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------
# the cases as host specs (tests/test_closed_loop_oracle_host.py runs them without a device)
# ---------------------------------------------------------------------------------------------
def _risk_kw(params):
    return dict(radii=(params.robot_radius, params.obstacle_radius), alpha=params.alpha,
                delta=params.delta, epsilon=params.epsilon)


def single_spec(device, case):
    """(LoopSpec, x0 [1, nx]) of a single-loop case; ``device`` may be the CPU."""
    c = single.CONFIGS[SINGLE_CASES[case]]
    _, nominal, x_ref, u_ref, x0, disturbance = single._setup(device)
    spec = clo.loop_spec(MODEL, _np(nominal), _np(x_ref), _np(u_ref), single.N, horizon=H, chol=CHOL,
                         metric=c["metric"], seed=single.SEED,
                         disturbance=_np(disturbance) if c["disturbed"] else None, step=c["step"],
                         stream_offset=OFFSET, **_risk_kw(RiskParams()))
    return spec, np.asarray(x0, dtype=np.float64)[None]


def batch_spec(device, case):
    """(LoopSpec, x0 [B, nx]) of a batch case; ``device`` may be the CPU."""
    _, nominal, x_ref, u_ref = base._setup(device)
    common = dict(horizon=H, n_problems=B, seed=base.SEED, disturbance=_np(base._disturbance(device)),
                  stream_offset=OFFSET)
    if case == "B1":
        spec = clo.loop_spec(MODEL, _np(nominal), _np(x_ref), _np(u_ref), base.N, chol=CHOL,
                             metric="dr_cvar", **_risk_kw(RiskParams()), **common)
    else:
        x_ref, u_ref = route._routes(device)
        O, table = nominal.shape[0], route.TABLE
        schedule = noise._schedule(O)
        chol = np.array([[[schedule.factor(b * O + o, t) for t in range(H)] for o in range(O)]
                         for b in range(B)])
        spec = clo.loop_spec(MODEL, _np(nominal), _np(x_ref), _np(u_ref), base.N, chol=chol,
                             metric=route.NAMES, draw_period=BATCH_CASES[case],
                             radii=(table.robot_radius, table.obstacle_radius), alpha=table.alpha,
                             delta=table.delta, epsilon=table.epsilon, **common)
    return spec, base._x0()


def _batch_loop(device, case, steps_per_graph=1):
    model, nominal, x_ref, u_ref = base._setup(device)
    kw = dict(n_problems=B, seed=base.SEED, disturbance=base._disturbance(device),
              steps_per_graph=steps_per_graph)
    if case == "B1":
        return RecedingHorizonBatch(model, nominal, x_ref, u_ref, base.N, RiskParams(), metric="dr_cvar", **kw)
    x_ref, u_ref = route._routes(device)
    return RecedingHorizonBatch(model, nominal, x_ref, u_ref, base.N, route.TABLE, metric=route.NAMES,
                                noise=noise._schedule(nominal.shape[0]), draw_period=BATCH_CASES[case], **kw)


@functools.lru_cache(maxsize=None)
def _batch_reference(device, case):
    """The reference backend's 12 steps of a batch case: (result on the host, per-step trace)."""
    loop = _batch_loop(device, case)
    result = base._run(loop, base._x0(), "reference")
    return result, [tuple(t.cpu() for t in row) for row in loop.reference_trace]


# ---------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------
def _fallback_memory(trace_u, solved, i):
    """The device's fallback memory at step i: the trace u of the last solved step before i."""
    before = np.flatnonzero(solved[:i])
    return trace_u[before[-1]] if before.size else None


def _certify(spec, x0, states, inputs, info, trace, label, require_solved):
    """Every step of every problem of one run; arrays carry a leading problem dimension, ``trace``
    is (x [B, n, H + 1, nx], u [B, n, H, nu], info [B, n, 10]).  Returns the printed figures."""
    tx, tu, tinfo = trace
    Bn, n = inputs.shape[:2]
    nx, nu = spec.A.shape[0], spec.B.shape[1]
    assert states.shape == (Bn, n + 1, nx) and tx.shape == (Bn, n, H + 1, nx) and tu.shape == (Bn, n, H, nu)
    np.testing.assert_array_equal(states[:, 0], x0, err_msg=label)
    status = tinfo[..., _native.MPC_INFO_STATUS]
    solved = np.isin(status, SOLVED)
    polished = tinfo[..., _native.MPC_INFO_POLISHED] == 1
    if require_solved:
        assert solved.all(), (label, status)
    (u_lo, u_hi), (p_lo, p_hi) = (np.asarray(b, dtype=np.float64) for b in (spec.u_bounds, spec.p_bounds))
    worst_u = 0.0
    for b in range(Bn):
        for i in range(n):
            tag = f"{label} problem {b} step {i}"
            x, u, inf = tx[b, i], tu[b, i], tinfo[b, i]
            # the answer alone
            assert x[0].tobytes() == states[b, i].tobytes(), tag
            assert np.all(np.isfinite(x)) and np.all(np.isfinite(u)), tag
            err = np.abs(x.astype(np.longdouble) - clo.rollout_ld(spec.A, spec.B, x[0], u))[1:].max()
            roll_tol = 64 * (H * nu + nx) * 2.0 ** -53 * max(1.0, np.abs(x).max())
            assert err <= roll_tol, (tag, float(err), roll_tol)
            if solved[b, i]:   # (a fallback rollout is bound by no box: module docstring)
                pos = x[1:] @ spec.C.T
                assert np.all(u >= u_lo - MPC_TOL) and np.all(u <= u_hi + MPC_TOL), (tag, u.min(0), u.max(0))
                assert np.all(pos >= p_lo - MPC_TOL) and np.all(pos <= p_hi + MPC_TOL), (tag, pos.min(0), pos.max(0))
            # the advance
            assert inputs[b, i].tobytes() == u[0].tobytes(), tag
            assert info[b, i].tobytes() == inf.tobytes(), tag
            want = x[1] + spec.disturbance[b, i] if spec.disturbance is not None else x[1]
            assert states[b, i + 1].tobytes() == want.tobytes(), tag
            if solved[b, i]:
                assert inf[_native.MPC_INFO_USED_FALLBACK] == 0, tag
                a = clo.step(spec, i, b, states[b, i])
                assert a.status == "optimal" and max(a.kkt.values()) < 1e-8, (tag, a.status, a.kkt)
                tol = MPC_TOL if polished[b, i] else UNPOLISHED_TOL
                worst_u = max(worst_u, float(np.abs(u - a.u).max()))
                np.testing.assert_allclose(u, a.u, rtol=0, atol=tol, err_msg=tag)
                np.testing.assert_allclose(x, a.x, rtol=0, atol=tol, err_msg=tag)
                if polished[b, i]:
                    assert abs(inf[_native.MPC_INFO_OBJECTIVE] - a.objective) <= 1e-6 * max(1.0, abs(a.objective)), tag
                    assert abs(inf[_native.MPC_INFO_MAX_SLACK] - max(a.slacks.max(initial=0.0), 0.0)) < 1e-6, tag
            else:
                assert inf[_native.MPC_INFO_USED_FALLBACK] == 1, tag
                u_ref_window = spec.u_ref[b][clo.window_rows(spec, i, H)]
                want_u = mpc_qp.fallback_inputs(H, nu, u_ref_window, _fallback_memory(tu[b], solved[b], i))
                assert u.tobytes() == np.ascontiguousarray(want_u).tobytes(), (tag, np.abs(u - want_u).max())
                np.testing.assert_allclose(x, mpc_qp.rollout(spec.A, spec.B, x[0], u), rtol=0, atol=1e-12,
                                           err_msg=tag)
    share = polished[solved].mean() if solved.any() else float("nan")
    print(f"{label}: solved {int(solved.sum())} / {solved.size}, polished share of solved {share:.3f}, "
          f"largest |u - u_oracle| {worst_u:.2e}")
    return solved


def _status_of_last_step(loop, n):
    """The loop's halfspace entry launched once more on the state of the last step run, with a
    status buffer: (record, status) as numpy.  Single loops and the RiskParams batch use the plain
    device-state entry, the B2 batch the noise entry."""
    dev = loop.model.device
    state = torch.tensor([OFFSET + n - 1, loop._step - 1], dtype=torch.int64).to(dev)
    units = loop._record.shape[0] * H
    status = torch.full((units,), -1, dtype=torch.int32, device=dev)
    if getattr(loop, "noise", None) is not None:
        out, _ = engine.sampled_halfspaces_noise(
            loop.nominal_path, loop.ego_path, loop.n_obstacles, H, loop.n_samples, loop.params, loop.metrics,
            state, loop.noise, draw_period=loop.draw_period, seed=loop.seed,
            zero_first_step=loop.zero_first_step, status=status)
    else:
        assert getattr(loop, "_risk_table", None) is None and getattr(loop, "_codes", None) is None
        out = engine.sampled_halfspaces_dev(loop.nominal_path, loop.ego_path, H, loop.n_samples, loop.params,
                                            state, noise_cov=loop.noise_cov, seed=loop.seed,
                                            zero_first_step=loop.zero_first_step, status=status)
    return _np(out), _np(status)


def _check_records(spec, loop, x0, label):
    """Graph runs of 1, 5 and 12 steps in all: after each the loop's record (and selected) buffer
    against the host record of the last step run.  Returns the largest error over its tolerance."""
    O, Bn = spec.n_obstacles, spec.n_problems
    loop.reset(x0, step=spec.step, stream_offset=OFFSET)
    done, worst = 0, 0.0
    for n in RECORD_RUNS:
        loop.run(n - done, backend="graph")
        done = n
        got = _np(loop._record).reshape(Bn, O * H, 8)
        again, status = _status_of_last_step(loop, n)
        assert again.tobytes() == _np(loop._record).tobytes(), (label, n)
        assert np.all(status == _native.UNIT_OK), (label, n, status)
        selected = getattr(loop, "_selected", None)
        for b in range(Bn):
            ref, tol = clo.step_record(spec, n - 1, b)
            assert ref.ok.all() and tol.max() < OFFSET_TOL, (label, n, b, tol.max())
            err = np.abs(got[b] - ref.rec)
            worst = max(worst, float((err / tol).max()))
            assert np.all(err <= tol), (f"{label} after {n} steps, problem {b}: unit, column "
                                        f"{np.argwhere(err > tol)[:4].tolist()}, error / tolerance "
                                        f"{(err / tol).max():.3g}")
            if selected is not None:
                sel = _np(selected).reshape(Bn, O * H, engine.SELECTED_WIDTH)[b]
                ch, cg = clo.METRIC_COLUMNS[spec.metrics[b]]
                assert sel[:, :3].tobytes() == np.ascontiguousarray(got[b][:, [ch, ch + 1, cg]]).tobytes(), (label, n, b)
                assert np.all(sel[:, 3] == 0.0), (label, n, b)
    print(f"{label}: largest record error / tolerance {worst:.3f} over runs of {RECORD_RUNS} steps")
    return worst


@pytest.mark.parametrize("case", list(SINGLE_CASES))
def test_single_loop_steps_match_the_host_oracle(dev, case):
    name = SINGLE_CASES[case]
    c = single.CONFIGS[name]
    spec, x0 = single_spec(dev, case)
    (states, inputs, info), want, trace = single._reference(dev, **c)
    trace = tuple(np.stack([_np(row[k]) for row in trace])[None] for k in range(3))
    solved = _certify(spec, x0, _np(states)[None], _np(inputs)[None], _np(info)[None], trace, case,
                      require_solved=case in ALL_SOLVED)
    if case not in ALL_SOLVED:
        # solved and unsolved steps both occur; an unsolved step before the first solved one rolls
        # out the u_ref window, one after it the remembered optimum (S3_cap3 and S3_mean reach the
        # first branch, S3_cap4 the second: tests/test_closed_loop_gpu.py's docstring)
        assert solved.any() and (~solved).any(), solved
        first = int(np.argmax(solved[0]))
        print(f"{case}: unsolved steps without a remembered optimum {int((~solved[0, :first]).sum())}, "
              f"with one {int((~solved[0, first:]).sum())}")
    # what was certified is the graph path's output too
    loop = single._loop(dev, c["metric"], c["disturbed"], 3, max_iter=c["max_iter"])
    loop.reset(single._setup(dev)[4], step=c["step"], stream_offset=OFFSET)
    got = single._bytes(tuple(t.cpu() for t in loop.run(STEPS, backend="graph")))
    for what, g, w in zip(("states", "inputs", "info"), got, want):
        assert g == w, f"{case}: graph {what} differ from the reference backend's"


@pytest.mark.parametrize("case", list(BATCH_CASES))
def test_batch_steps_match_the_host_oracle(dev, case):
    spec, x0 = batch_spec(dev, case)
    (states, inputs, info), trace = _batch_reference(dev, case)
    trace = tuple(np.stack([_np(row[k]) for row in trace], axis=1) for k in range(3))
    _certify(spec, x0, _np(states), _np(inputs), _np(info), trace, case, require_solved=True)
    got = base._run(_batch_loop(dev, case, 3), base._x0(), "graph")
    for what, g, w in zip(("states", "inputs", "info"), base._bytes(got), base._bytes((states, inputs, info))):
        assert g == w, f"{case}: graph {what} differ from the reference backend's"


@pytest.mark.parametrize("case", ["S1_dr_cvar", "S2", "B1", "B2_period1", "B2_independent"])
def test_record_buffers_match_the_host_record(dev, case):
    """The records do not depend on the metric or the solver's cap, so S1's dr_cvar run stands for
    the mean and the capped runs on the same draws."""
    if case in SINGLE_CASES:
        c = single.CONFIGS[SINGLE_CASES[case]]
        spec, x0 = single_spec(dev, case)
        loop = single._loop(dev, c["metric"], c["disturbed"], 1)
        _check_records(spec, loop, x0[0], case)
    else:
        spec, x0 = batch_spec(dev, case)
        _check_records(spec, _batch_loop(dev, case), x0, case)
