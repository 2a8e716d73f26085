"""The receding-horizon safety-filter loop on the device, replayed from one graph.

The reference simulates 30 s (``config/parameters.py``: ``SIM_TIME = 30.0``, ``DT = 0.2``) but
``main.py:95-118`` filters only the first window; ``MPCSafetyFilter._fallback``
(``core/mpc_filter.py:197-210``) shifts ``last_optimal_u`` by one step, which is what a caller of
``filter_trajectory`` once per control step needs.  :class:`RecedingHorizonFilter` is that caller:
at every step the filter is re-solved from the current state against freshly drawn obstacle
predictions.  One control step is three launches on one stream,

1. ``drcvar_sampled_halfspaces_f64_dev`` — the window's halfspaces from the nominal paths, the
   window start and the stream offset read from a 16-byte device state;
2. ``drcvar_mpc_filter_f64_ex`` — the QP (and the fallback rollout when it is not solved);
3. ``drcvar_mpc_step_advance_f64`` — applies the first input, logs the step, keeps the fallback
   memory, writes the next ``x0`` / reference window / fallback inputs and advances the state,

so a captured step carries no frozen per-step quantity and ``run`` replays one graph per control
step (or per ``steps_per_graph`` steps) with no host work in between.  Exact semantics:
``include/drcvar_mpc.h`` (``drcvar_mpc_step_advance_f64``) and DESIGN.md §5.3.

By default (``linearize="reference"``) the halfspaces are computed about the REFERENCE path
(``ego_path = x_ref_path @ C.T``), as the reference does for its one window (``main.py:95-97``),
not about the actual state.  With ``linearize="predicted"`` the halfspace launch is
``drcvar_sampled_halfspaces_f64_pred`` (``include/drcvar_loop_pred.h``) and every
loop's halfspaces are taken about its OWN motion: window row 0 about the state actually reached
(disturbance included), row t >= 1 about the previous step's predicted state for the same path
time (the solver's ``x_out``, shifted by one row; the rolled-out fallback after a failed solve;
the reference path on the first step after ``reset``).  ``relinearize=r`` then repeats
(halfspaces about the answer just written, solve) r times before the advance, on the same draws:
a control step is ``3 + 2 r`` launches, still one linear chain.  One problem per loop;
:class:`RecedingHorizonBatch` advances B loops in lockstep with the same launches per step
(``drcvar_mpc_step_advance_batch_f64``, ``include/drcvar_loop.h``: one workgroup and one device
state per problem).

Both classes take ``evaluate=LoopEvaluation(...)``: a fourth launch per control step
(``drcvar_loop_clearance_f64``, ``include/drcvar_loop_eval.h``) then holds the state just reached
against M noise realisations of the obstacles and keeps the running minimum clearance and the
per-step collision counts on the device; ``safety()`` returns them.  With
``evaluate=None`` a step is the three launches above and nothing else changes.

:class:`RecedingHorizonBatch` also takes ``params=engine.RiskTable(...)``: every loop then filters
with its OWN (alpha, delta, epsilon), launch 1 being ``drcvar_sampled_halfspaces_f64_risk``
(``include/drcvar_loop_risk.h``), and ``draw_period=D`` gives problems ``b`` and
``b + D`` the same draws, so a grid of settings x D replicates is one batch on common random
numbers.  With a ``RiskParams`` nothing changes.

``RecedingHorizonBatch(metric=[...])``, one name per problem, gives every loop its OWN metric:
launch 1 is then ``drcvar_sampled_halfspaces_f64_metric`` (``include/drcvar_loop_metric.h``,
DESIGN.md §5.8), the risk-table launch whose storing lane also writes each unit's chosen halfspace,
and the solve reads those: mean, CVaR and DR-CVaR are compared on common random numbers in one
batch.  With a string metric nothing changes.
"""
from __future__ import annotations

import ctypes
import dataclasses

import torch

from .. import _native, engine
from ..evaluation import metrics, monte_carlo
from ..core.mpc_filter import (DEFAULT_MAX_ITER, DEFAULT_TOL, METRIC_COLUMNS, MPCModel, filter_batch,
                               record_views)
from ..engine import DEFAULT_NOISE_COV
from .obstacles import NOISE_COV

BACKENDS = ("graph", "launches", "reference")
LINEARIZE = ("reference", "predicted")
_MASK64 = 2 ** 64 - 1
_MIN_LOG_ROWS = 64


def _signed64(v: int) -> int:
    """The two's-complement int64 with the bit pattern of ``v mod 2^64``."""
    v &= _MASK64
    return v - 2 ** 64 if v >= 2 ** 63 else v


def check_run_steps(n_steps: int, steps_per_graph: int, backend: str) -> None:
    """``run``'s argument checks (host only)."""
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")
    if int(n_steps) < 0:
        raise ValueError(f"n_steps={n_steps} must not be negative")
    if backend == "graph" and int(n_steps) % int(steps_per_graph) != 0:
        raise ValueError(f"n_steps={n_steps} is not a multiple of steps_per_graph={steps_per_graph}")


def _capture_chain(dev, make_step, mutable, steps_per_graph):
    """``steps_per_graph`` steps of ``make_step(stream)`` captured on one explicit stream: one
    linear chain, no branches.  One eager step runs first on that stream (every kernel's code
    object is loaded before the capture begins); the buffers it advanced (``mutable()``) are put
    back."""
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    step = make_step(side)
    with torch.cuda.stream(side):
        saved = [t.clone() for t in mutable()]
        step()
        for t, s in zip(mutable(), saved):
            t.copy_(s)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(steps_per_graph):
            step()
    return graph


@dataclasses.dataclass(frozen=True)
class LoopEvaluation:
    """Out-of-sample collision evaluation of a loop while it runs (``evaluate=`` of the two loop
    classes): every control step also updates, on the device, the running minimum
    clearance of each loop against ``n_realizations`` noise realisations of its obstacles and the
    per-step collision counts (``drcvar_loop_clearance_f64``, ``include/drcvar_loop_eval.h``).

    The realisations are those of ``evaluation.monte_carlo.min_clearance_device`` for (``noise``,
    ``noise_cov``, ``seed``, ``stream_offset`` [+ b with ``independent_problems``], O obstacles,
    ``T = noise_steps`` steps, default the paths' P rows, noise-free path row 0): a loop at path
    row s meets realisation m's obstacles of step s.  ``independent_problems=False`` gives every
    problem of a batch the same realisations (common random numbers across loops)."""

    n_realizations: int
    noise: str = "laplace"
    noise_cov: object = NOISE_COV
    robot_radius: float = None
    obstacle_radius: float = None
    seed: int = 0
    stream_offset: int = 0
    independent_problems: bool = True
    noise_steps: int = None

    def validate(self):
        """Host-only argument checks; returns ``self``."""
        if isinstance(self.n_realizations, bool) or int(self.n_realizations) != self.n_realizations \
                or not 1 <= int(self.n_realizations) <= 2 ** 40:
            raise ValueError(f"n_realizations={self.n_realizations!r} must be an integer in 1..2^40")
        monte_carlo._noise_params(self.noise, self.noise_cov)       # raises on an unknown kind
        for name in ("robot_radius", "obstacle_radius"):
            v = getattr(self, name)
            if v is None or not float(v) >= 0.0:
                raise ValueError(f"{name}={v!r} must be given and must not be negative")
        if self.noise_steps is not None and int(self.noise_steps) < 1:
            raise ValueError(f"noise_steps={self.noise_steps} must be at least 1 (or None: the paths' rows)")
        return self

    @property
    def combined_radius(self):
        return float(self.robot_radius) + float(self.obstacle_radius)


def check_evaluated_steps(first, last, noise_steps):
    """An evaluated loop may only visit path rows ``0 <= s < noise_steps`` (host only): a loop
    never silently stops being evaluated."""
    if first < 0 or last >= noise_steps:
        raise ValueError(f"an evaluated loop visits path rows {first}..{last}, outside the "
                         f"evaluation's 0..{noise_steps - 1} (LoopEvaluation.noise_steps)")


def check_evaluate(evaluate):
    """The ``evaluate=`` argument of the loop classes (host only)."""
    if evaluate is not None:
        if not isinstance(evaluate, LoopEvaluation):
            raise ValueError("evaluate must be a LoopEvaluation or None")
        evaluate.validate()


class _Evaluated:
    """What the two loop classes share for ``evaluate=``: the buffers, the launch appended to a
    control step, and :meth:`safety`.  The single class is the batch of one problem here
    (``_eval_B = 1``; its ``[...]`` buffers are viewed with a leading problem dimension)."""

    evaluate = None

    def _eval_init(self, evaluate, n_problems, n_obstacles, nominal_flat):
        self.evaluate = evaluate
        self._eval_B, self._eval_O, self._eval_nominal = n_problems, n_obstacles, nominal_flat
        self._eval_hits = None
        if evaluate is None:
            return
        self._noise_steps = int(evaluate.noise_steps) if evaluate.noise_steps is not None \
            else self.path_steps
        self._eval_C = torch.as_tensor(self.model.C, dtype=torch.float64).reshape(2, self.model.nx)
        self._min_d2 = torch.full((n_problems, int(evaluate.n_realizations)), float("inf"),
                                  dtype=torch.float64, device=self.model.device)
        self._eval_history, self._eval_mode, self._eval_first = [], None, 0

    def _eval_batched(self, t):
        """A per-problem buffer with its leading problem dimension."""
        return t if isinstance(self, RecedingHorizonBatch) else t.unsqueeze(0)

    def _eval_launch(self, stream):
        ev = self.evaluate
        return monte_carlo.prepare_loop_clearance_step(
            self._x0, self._eval_C.numpy(), self._eval_nominal, self._eval_O,
            self._state.view(self._eval_B, 2), self._min_d2, self._eval_hits,
            step_begin=self._step_begin, log_rows=self._cap, noise_steps=self._noise_steps,
            noise=ev.noise, noise_cov=ev.noise_cov, robot_radius=ev.robot_radius,
            obstacle_radius=ev.obstacle_radius, seed=ev.seed, eval_offset=ev.stream_offset,
            problem_offset_stride=1 if ev.independent_problems else 0, zero_first_step=True,
            stream=stream)

    def _eval_rebase(self, cap, carry):
        """New per-step counts with the new logs; with ``carry`` (a rebase inside a run) row 0
        takes over the old table's count of the current state, as ``x_log``'s row 0 is the current
        state, and the rows before it are remembered for the ``reference`` backend."""
        if self.evaluate is None:
            return
        old, i = self._eval_hits, getattr(self, "_i", 0)
        self._eval_hits = torch.zeros((self._eval_B, cap + 1), dtype=torch.int64,
                                      device=self.model.device)
        if carry and old is not None:
            self._eval_hits[:, 0].copy_(old[:, i])
            self._eval_history.append(self._eval_batched(self._logs[0])[:, :i].clone())

    def _eval_reset(self):
        """After ``reset`` has settled the logs: +inf, zero counts, and the initial state (log row
        0) evaluated by one eager launch."""
        if self.evaluate is None:
            return
        self._min_d2.fill_(float("inf"))
        self._eval_hits.zero_()
        self._eval_history, self._eval_mode, self._eval_first = [], None, self._step
        self._eval_launch(torch.cuda.current_stream(self.model.device))()

    def _eval_check_run(self, n, backend):
        if self.evaluate is None:
            return
        check_evaluated_steps(self._step, self._step + int(n), self._noise_steps)
        mode = "reference" if backend == "reference" else "device"
        if int(n) > 0:
            if getattr(self, "_eval_mode", None) not in (None, mode):
                raise ValueError("an evaluated loop cannot mix the reference backend with the "
                                 "device backends between two resets")
            self._eval_mode = mode

    def _reference_safety(self):
        """(min_clearance [B, M], step_hits [B, rows]) after the fact, from entries that predate
        the loop form: per problem one ``min_clearance_device`` call (K = 1, T = noise_steps) on an
        ego whose visited rows hold the logged positions and whose other rows lie 1e3 away from
        every obstacle's nominal row."""
        ev, dev = self.evaluate, self.model.device
        Tn, O, M = self._noise_steps, self._eval_O, int(ev.n_realizations)
        x_log = self._eval_batched(self._logs[0])
        states = torch.cat(self._eval_history + [x_log[:, :self._i + 1]], dim=1)
        pos = states @ self._eval_C.to(dev).T                                   # [B, visited, 2]
        first = self._eval_first
        rows = torch.arange(Tn, device=dev).clamp_(max=self.path_steps - 1)
        clearance, hits = [], []
        for b in range(self._eval_B):
            nominal = self._eval_nominal[b * O:(b + 1) * O].index_select(1, rows)   # [O, Tn, 2]
            ego = torch.stack((nominal[..., 0].max(dim=0).values + 1e3, nominal[0, :, 1]), dim=1)
            ego[first:first + pos.shape[1]] = pos[b]
            offset = ev.stream_offset + (b if ev.independent_problems else 0)
            c, h = monte_carlo.min_clearance_device(
                ego[None], nominal, M, noise=ev.noise, noise_cov=ev.noise_cov,
                robot_radius=ev.robot_radius, obstacle_radius=ev.obstacle_radius, seed=ev.seed,
                stream_offset=offset, zero_first_step=True, step_hits=True)
            clearance.append(c[0])
            hits.append(h[0, self._step_begin:self._step_begin + self._i + 1])
        return torch.stack(clearance), torch.stack(hits)

    def safety(self):
        """The safety statistics since ``reset``, device tensors (the single class drops the
        leading problem dimension): ``min_clearance [B, M]`` = sqrt(min d^2) - R, ``collided [B]``
        the fraction of realisations in collision at some visited state, ``step_hits [B, rows]``
        and ``step_collision_rate`` for the states since the last rebase (row 0: the state the
        logs start from), and ``metrics``, ``evaluation.metrics.safety_metrics`` per problem.  A
        problem with a NaN clearance has ``collided`` NaN (:func:`safety_statistics`)."""
        if self.evaluate is None:
            raise RuntimeError("the loop was built without evaluate=")
        if not self._primed:
            raise RuntimeError("call reset(x0) before safety()")
        R = self.evaluate.combined_radius
        if self._eval_mode == "reference":
            clearance, hits = self._reference_safety()
            result = safety_statistics(None, hits, R, clearance=clearance)
        else:
            result = safety_statistics(self._min_d2, self._eval_hits[:, :self._i + 1].clone(), R)
        if not isinstance(self, RecedingHorizonBatch):
            result = {k: v[0] for k, v in result.items()}
        return result


def safety_statistics(min_d2, hits, R, clearance=None):
    """What ``safety()`` reports, from the evaluation's accumulators alone (tensors on any device):
    ``min_d2 [B, M]`` the running minimum of the squared distance, ``hits [B, rows]`` the per-step
    counts, ``R`` the combined radius.  ``clearance [B, M]`` given (the reference mode, which has
    clearances and no squared distances): a realisation collided when its clearance is negative.

    A NaN clearance (a non-finite position met the evaluation kernel, which propagates it) makes
    problem b's sample undefined: ``collided[b]`` is NaN, as ``metrics`` are, never a rate over the
    realisations that happen to be comparable.  Other problems are untouched."""
    if clearance is None:
        clearance = torch.sqrt(min_d2) - R
        collided = min_d2 < R * R
    else:
        collided = clearance < 0
    f64 = dict(dtype=torch.float64, device=clearance.device)
    M = torch.full((), float(clearance.shape[1]), **f64)   # a tensor divisor (monte_carlo.py)
    rate = collided.sum(dim=1).to(torch.float64) / M
    undefined = torch.isnan(clearance).any(dim=1)
    return {"min_clearance": clearance,
            "collided": torch.where(undefined, torch.full_like(rate, float("nan")), rate),
            "step_hits": hits, "step_collision_rate": hits.to(torch.float64) / M,
            "metrics": [metrics.safety_metrics(row) for row in clearance]}


def check_linearize(linearize, relinearize):
    """The ``linearize=`` / ``relinearize=`` arguments of the loop classes (host only)."""
    if linearize not in LINEARIZE:
        raise ValueError(f"linearize must be one of {LINEARIZE}, got {linearize!r}")
    if isinstance(relinearize, bool) or int(relinearize) != relinearize or int(relinearize) < 0:
        raise ValueError(f"relinearize={relinearize!r} must be a non-negative integer")
    if int(relinearize) > 0 and linearize != "predicted":
        raise ValueError('relinearize > 0 needs linearize="predicted"')


def check_risk(params, draw_period, n_problems, linearize):
    """The ``params=`` / ``draw_period=`` arguments of the loop classes (host only).  Returns the
    draw period of a :class:`engine.RiskTable` (``None`` = ``n_problems``), and None for a
    ``RiskParams``; ``n_problems=None`` is the single-loop class, which takes no table."""
    if not isinstance(params, engine.RiskTable):
        if draw_period is not None:
            raise ValueError("draw_period needs params=RiskTable(...): a RiskParams batch draws "
                             "every problem's own units")
        return None
    if n_problems is None:
        raise ValueError("a RiskTable belongs to RecedingHorizonBatch; RecedingHorizonFilter takes "
                         "a RiskParams")
    if linearize == "predicted":
        raise ValueError('a RiskTable cannot be combined with linearize="predicted"')
    params.validate()
    if len(params) != int(n_problems):
        raise ValueError(f"the RiskTable has {len(params)} rows, n_problems={n_problems}")
    if draw_period is None:
        return int(n_problems)
    if isinstance(draw_period, bool) or int(draw_period) != draw_period or int(draw_period) < 1:
        raise ValueError(f"draw_period={draw_period!r} must be a positive integer or None")
    return int(draw_period)


def check_metric(metric, n_problems, linearize):
    """The ``metric=`` argument of the loop classes (host only).  A name returns None (today's
    path); a sequence of ``n_problems`` names returns them as a tuple; ``n_problems=None`` is the
    single-loop class, which takes a name only."""
    if isinstance(metric, str):
        if metric not in METRIC_COLUMNS:
            raise ValueError(f"metric must be one of {tuple(METRIC_COLUMNS)}, got {metric!r}")
        return None
    try:
        names = tuple(metric)
    except TypeError:
        raise ValueError(f"metric must be one of {tuple(METRIC_COLUMNS)} or a sequence of them, "
                         f"got {metric!r}") from None
    if n_problems is None:
        raise ValueError("a sequence of metrics belongs to RecedingHorizonBatch; "
                         "RecedingHorizonFilter takes one name")
    if linearize == "predicted":
        raise ValueError('a sequence of metrics cannot be combined with linearize="predicted"')
    if len(names) != int(n_problems):
        raise ValueError(f"metric has {len(names)} names, n_problems={n_problems}")
    for name in names:
        if not isinstance(name, str) or name not in engine.METRIC_CODES:
            raise ValueError(f"metric names must be among {tuple(engine.METRIC_CODES)}, got {name!r}")
    return names


class _Linearized:
    """What the two loop classes share for ``linearize="predicted"``: the
    halfspaces of window row t are taken about the loop's own prediction for that path time
    instead of the reference path (``drcvar_sampled_halfspaces_f64_pred``,
    ``include/drcvar_loop_pred.h``).  The single class is the batch of one problem here."""

    linearize, relinearize = "reference", 0

    def _lin_init(self, linearize, relinearize, n_problems, n_obstacles, nominal_flat):
        self.linearize, self.relinearize = linearize, int(relinearize)
        self._lin_B, self._lin_O, self._lin_nominal = n_problems, n_obstacles, nominal_flat
        C = torch.as_tensor(self.model.C, dtype=torch.float64).reshape(2, self.model.nx)
        self._lin_C = C.contiguous().numpy()          # host memory: copied into each launch
        self._lin_C_dev = C.to(self.model.device)

    def _lin_prime(self):
        """``reset``: the prediction the first step linearises about is the reference path, row j
        of ``x_out`` holding ``x_ref_path[c(step - 1 + j)]`` (``shift = 1`` reads row t + 1)."""
        if self.linearize == "predicted":
            self._x.copy_(self._window(self.x_ref_path, self._step - 1, self.model.horizon + 1))

    def _lin_launch(self, stream, shift):
        """The halfspace launch of a captured step about (``x0``, ``x_out``)."""
        return engine.prepare_sampled_halfspaces_pred(
            self._lin_nominal, self._x0.view(self._lin_B, -1), self._x, self._lin_C, self._lin_O,
            self.model.horizon, self.n_samples, self.params, self._state.view(-1, 2)[0],
            shift=shift, noise_cov=self.noise_cov, seed=self.seed,
            zero_first_step=self.zero_first_step, out=self._record, stream=stream, chol=self.chol)[0]

    def _lin_reference_record(self, window, shift):
        """The same record ``[B O, H, 8]`` from entries that predate the predicted form: per
        problem the ego is formed by a torch multiply-and-add chain over the states (from +0.0, in
        the kernel's order) and ``engine.sampled_halfspaces`` runs on the problem's unit window.
        Bitwise the kernel's fma chain when every product ``c_out[i, j] * x[j]`` is exact (a
        selector ``C``, the reference's model, or power-of-two entries); otherwise it agrees to an
        ulp of the ego."""
        H, B, O = self.model.horizon, self._lin_B, self._lin_O
        rows = (self._rows[H] + shift).clamp_(max=H)
        records = []
        for b in range(B):
            xs = self._x[b].index_select(0, rows)                 # [H, nx]: pred[b, min(t + shift, H)]
            xs[0].copy_(self._x0.view(B, -1)[b])                  # t = 0: the state actually reached
            ego = torch.zeros((H, 2), dtype=torch.float64, device=xs.device)
            for j in range(xs.shape[1]):
                ego = ego + xs[:, j:j + 1] * self._lin_C_dev[:, j]
            records.append(engine.sampled_halfspaces(
                window, ego, self.n_samples, self.params, noise_cov=self.noise_cov, chol=self.chol,
                seed=self.seed, stream_offset=self._offset, zero_first_step=self.zero_first_step,
                unit_begin=b * O * H, unit_count=O * H))
        return torch.cat(records).view(B * O, H, engine.OUT_WIDTH)


class RecedingHorizonFilter(_Evaluated, _Linearized):
    """One problem's receding-horizon loop.

    ``nominal_path [O, P, 2]`` (obstacles), ``x_ref_path [P, nx]`` and ``u_ref_path [P, nu]`` are
    float64 tensors on ``model.device``; past row ``P - 1`` every path holds its last row.
    ``disturbance`` (optional ``[D, nx]`` device tensor): row ``i`` is added to the state after
    step ``i`` counted from :meth:`reset`; a run may then take at most ``D`` steps per reset.
    The other arguments are those of ``engine.sampled_halfspaces`` and ``filter_batch``.

    ``run(n, backend)`` returns ``(states [n + 1, nx], inputs [n, nu], info [n, 10])`` device
    tensors; ``states[0]`` is the state the run started from.  A failed solve (any status but
    optimal / optimal_inaccurate, cluster failures included) is a step whose fallback inputs were
    rolled out by the solver: it is recorded in ``info`` and the loop goes on, never synchronising.
    Backends: ``"graph"`` (captured on one explicit stream, one linear chain), ``"launches"`` (the
    same three launches issued eagerly) and ``"reference"`` (the semantics spelled out with
    ``engine.sampled_halfspaces`` on gathered windows, ``filter_batch`` and torch ops; the tests'
    yardstick; it also fills ``reference_trace`` with each step's solver outputs).

    ``linearize="predicted"`` takes the halfspaces about the loop's own state and predicted path
    (module docstring) and ``relinearize=r`` adds r passes of (halfspaces about the
    answer just written, solve) per step, all on the step's draws; the logged ``info`` is the last
    pass's.  Its ``reference`` backend forms the ego by a torch multiply-and-add chain, which is
    bitwise the kernel's fma chain when every product ``C[i, j] x[j]`` is exact (a selector ``C``,
    power-of-two entries) and agrees to an ulp of the ego otherwise.
    """

    def __init__(self, model: MPCModel, nominal_path, x_ref_path, u_ref_path, n_samples, params, *,
                 metric="dr_cvar", noise_cov=DEFAULT_NOISE_COV, chol=None, seed=0,
                 zero_first_step=True, max_iter=DEFAULT_MAX_ITER, tol=DEFAULT_TOL, polish=True,
                 options=None, disturbance=None, steps_per_graph=1, evaluate=None,
                 linearize="reference", relinearize=0):
        check_metric(metric, None, linearize)       # (a sequence of metrics is the batch class's)
        if int(steps_per_graph) < 1:
            raise ValueError(f"steps_per_graph={steps_per_graph} must be at least 1")
        check_evaluate(evaluate)
        check_linearize(linearize, relinearize)
        check_risk(params, None, None, linearize)   # (a RiskTable is the batch class's)
        n = int(n_samples)
        if n < 1 or n > _native.MAX_SAMPLES:
            raise ValueError(f"n_samples={n} outside 1..{_native.MAX_SAMPLES}")
        params.validate()
        dev = model.device
        H, nx, nu = model.horizon, model.nx, model.nu
        if not isinstance(nominal_path, torch.Tensor) or nominal_path.dim() != 3:
            raise ValueError("nominal_path must be a float64 [O, P, 2] tensor")
        engine.check_path(nominal_path, "nominal_path", (None, None, 2))
        P = nominal_path.shape[1]
        engine.check_path(x_ref_path, "x_ref_path", (P, nx))
        engine.check_path(u_ref_path, "u_ref_path", (P, nu))
        if disturbance is not None:
            engine.check_path(disturbance, "disturbance", (None, nx))
        for t, name in ((nominal_path, "nominal_path"), (x_ref_path, "x_ref_path"),
                        (u_ref_path, "u_ref_path"), (disturbance, "disturbance")):
            if t is not None and t.device != dev:
                raise ValueError(f"{name} must live on the model's device {dev}, got {t.device}")
        self.model, self.params, self.metric = model, params, metric
        self.n_samples, self.seed = n, int(seed) & _MASK64
        self.noise_cov, self.chol, self.zero_first_step = noise_cov, chol, bool(zero_first_step)
        self.max_iter, self.tol, self.polish, self.options = int(max_iter), float(tol), bool(polish), options
        self.steps_per_graph = int(steps_per_graph)
        self.nominal_path = nominal_path
        self.x_ref_path = x_ref_path.contiguous()
        self.u_ref_path = u_ref_path.contiguous()
        self.disturbance = None if disturbance is None else disturbance.contiguous()
        self.path_steps = P
        C = torch.as_tensor(model.C).to(dev)
        self.ego_path = (self.x_ref_path @ C.T).contiguous()   # formed once
        O = nominal_path.shape[0]
        f64 = dict(dtype=torch.float64, device=dev)
        # the fixed buffers every captured launch reads or writes
        self._state = torch.zeros(2, dtype=torch.int64, device=dev)   # [stream_offset, step]
        self._x0 = torch.zeros((1, nx), **f64)
        self._x_ref_win = torch.zeros((1, H + 1, nx), **f64)
        self._u_fb = torch.zeros((1, H, nu), **f64)
        self._last_u = torch.zeros((H, nu), **f64)
        self._have_last = torch.zeros(1, dtype=torch.int32, device=dev)
        self._record = torch.zeros((O, H, engine.OUT_WIDTH), **f64)
        self._x = torch.zeros((1, H + 1, nx), **f64)
        self._u = torch.zeros((1, H, nu), **f64)
        self._info = torch.zeros((1, _native.MPC_INFO_WIDTH), **f64)
        self._workspace = torch.empty(max(model.workspace_doubles(1, O), 1), **f64)
        self._rows = {k: torch.arange(k, device=dev) for k in (H, H + 1)}
        self._eval_init(evaluate, 1, O, nominal_path)
        self._lin_init(linearize, relinearize, 1, O, nominal_path)
        self._logs = None           # (x_log [cap + 1, nx], u_log [cap, nu], info_log [cap, 10])
        self._cap, self._step_begin = 0, 0
        self._primed = False
        self._graph = None
        self._eager = {}
        self.reference_trace = []

    # ---- priming (torch ops, not a mode of the advance kernel) --------------------------------
    def _window(self, path, first, rows):
        idx = (self._rows[rows] + first).clamp_(0, self.path_steps - 1)
        return path.index_select(0, idx)

    def reset(self, x0, step=0, stream_offset=0):
        """Start a loop at path row ``step`` from state ``x0`` with the stream offset of its first
        draw: fills ``x0``, the first reference window and the first fallback inputs (the
        reference inputs: no optimum is remembered yet)."""
        dev = self.model.device
        H = self.model.horizon
        if self.evaluate is not None:
            check_evaluated_steps(int(step), int(step), self._noise_steps)
        x0 = torch.as_tensor(x0, dtype=torch.float64).reshape(1, self.model.nx).to(dev)
        self._step, self._offset = int(step), int(stream_offset) & _MASK64
        self._state.copy_(torch.tensor([_signed64(self._offset), self._step], dtype=torch.int64))
        self._x0.copy_(x0)
        self._x_ref_win[0].copy_(self._window(self.x_ref_path, self._step, H + 1))
        self._u_fb[0].copy_(self._window(self.u_ref_path, self._step, H))
        self._last_u.zero_()
        self._have_last.zero_()
        self._lin_prime()
        self._primed = True
        cap = max(self._cap, _MIN_LOG_ROWS) if self.disturbance is None else self.disturbance.shape[0]
        if self._logs is not None and cap == self._cap and self._step == self._step_begin:
            # the same first step and logs: what was captured stays valid
            for log in self._logs:
                log.fill_(float("nan"))
            self._logs[0][0].copy_(self._x0[0])
            self._i = 0
        else:
            self._rebase(cap)
        self._eval_reset()

    def _rebase(self, cap, carry=False):
        """New logs of ``cap`` rows whose row 0 is the current step (captured launches freeze the
        log pointers and the first step, so they are dropped)."""
        self._eval_rebase(cap, carry)
        nx, nu = self.model.nx, self.model.nu
        f64 = dict(dtype=torch.float64, device=self.model.device)
        nan = float("nan")
        rows = max(cap, 1)   # (never an empty allocation: the launches take the pointers)
        self._logs = (torch.full((cap + 1, nx), nan, **f64), torch.full((rows, nu), nan, **f64),
                      torch.full((rows, _native.MPC_INFO_WIDTH), nan, **f64))
        self._logs[0][0].copy_(self._x0[0])
        self._cap, self._i, self._step_begin = cap, 0, self._step
        self._graph = None
        self._eager = {}

    # ---- one control step as three launches on `stream` -----------------------------------------
    def _make_step(self, stream):
        m = self.model
        H = m.horizon
        again = None
        if self.linearize == "predicted":
            halfspaces = self._lin_launch(stream, 1)
            again = self._lin_launch(stream, 0) if self.relinearize else None
        else:
            halfspaces, _ = engine.prepare_sampled_halfspaces_dev(
                self.nominal_path, self.ego_path, H, self.n_samples, self.params, self._state,
                noise_cov=self.noise_cov, seed=self.seed, zero_first_step=self.zero_first_step,
                out=self._record, stream=stream, chol=self.chol)
        hs_h, hs_g = record_views(self._record, self.metric)
        vp = ctypes.c_void_p
        x_log, u_log, info_log = self._logs
        dist = self.disturbance
        advance = engine.PreparedLaunch(_native.lib().drcvar_mpc_step_advance_f64, (
            ctypes.pointer(m.model), vp(self._x.data_ptr()), vp(self._u.data_ptr()),
            vp(self._info.data_ptr()), vp(self.x_ref_path.data_ptr()), vp(self.u_ref_path.data_ptr()),
            self.path_steps, vp(dist.data_ptr() if dist is not None else None), self._step_begin,
            self._cap, vp(x_log.data_ptr()), vp(u_log.data_ptr()), vp(info_log.data_ptr()),
            vp(self._x0.data_ptr()), vp(self._x_ref_win.data_ptr()), vp(self._u_fb.data_ptr()),
            vp(self._last_u.data_ptr()), vp(self._have_last.data_ptr()), vp(self._state.data_ptr()),
            vp(int(stream.cuda_stream))), (self, x_log, u_log, info_log))
        out = (self._x, self._u, self._info)
        # with an evaluation: a fourth launch on the same stream, after the advance (x0 is then the
        # state just reached and state.step its path row); the chain stays linear
        evaluation = self._eval_launch(stream) if self.evaluate is not None else None

        def solve():
            filter_batch(m, hs_h, hs_g, self._x0, self._x_ref_win, self._u_fb, self.max_iter,
                         self.tol, self.polish, workspace=self._workspace, stream=stream,
                         options=self.options, out=out)

        def step():
            halfspaces()
            solve()
            # relinearize: the same draws (the state moves only in the advance) about the answer
            # just written, then the solve again; still one linear chain
            for _ in range(self.relinearize):
                again()
                solve()
            advance()
            if evaluation is not None:
                evaluation()
        return step

    def _mutable(self):
        evaluated = [] if self.evaluate is None else [self._min_d2, self._eval_hits]
        # (under "predicted" x_out is an input of the next step's halfspaces)
        predicted = [self._x] if self.linearize == "predicted" else []
        return [self._state, self._x0, self._x_ref_win, self._u_fb, self._last_u, self._have_last,
                *self._logs, *evaluated, *predicted]

    def _capture(self):
        return _capture_chain(self.model.device, self._make_step, self._mutable, self.steps_per_graph)

    # ---- the semantics, from the entry points that predate the loop -----------------------------
    def _reference_step(self, i):
        m = self.model
        H = m.horizon
        s = self._step
        window = self.nominal_path.index_select(
            1, (self._rows[H] + s).clamp_(0, self.path_steps - 1))
        for p in range(1 + self.relinearize):
            if self.linearize == "predicted":
                record = self._lin_reference_record(window, 1 if p == 0 else 0)
            else:
                ego_window = self._window(self.ego_path, s, H)
                record = engine.sampled_halfspaces(window, ego_window, self.n_samples, self.params,
                                                   noise_cov=self.noise_cov, chol=self.chol,
                                                   seed=self.seed, stream_offset=self._offset,
                                                   zero_first_step=self.zero_first_step)
            hs_h, hs_g = record_views(record[:, :H], self.metric)
            x, u, info = filter_batch(m, hs_h, hs_g, self._x0, self._x_ref_win, self._u_fb,
                                      self.max_iter, self.tol, self.polish, options=self.options)
            self._x.copy_(x)   # (the next linearisation point; the device backends' x_out)
        self.reference_trace.append((x[0].clone(), u[0].clone(), info[0].clone()))
        x_log, u_log, info_log = self._logs
        x_next = x[0, 1]
        if self.disturbance is not None:
            x_next = x_next + self.disturbance[i]
        x_log[i + 1].copy_(x_next)
        u_log[i].copy_(u[0, 0])
        info_log[i].copy_(info[0])
        status = info[0, _native.MPC_INFO_STATUS]
        solved = (status == _native.MPC_STATUS_OPTIMAL) | (status == _native.MPC_STATUS_OPTIMAL_INACCURATE)
        self._last_u.copy_(torch.where(solved, u[0], self._last_u))
        self._have_last.copy_(torch.where(solved, torch.ones_like(self._have_last), self._have_last))
        self._x0[0].copy_(x_next)
        self._x_ref_win[0].copy_(self._window(self.x_ref_path, s + 1, H + 1))
        plain = self._window(self.u_ref_path, s + 1, H)
        shifted = torch.cat((self._last_u[1:], plain[H - 1:]), dim=0)
        self._u_fb[0].copy_(torch.where(self._have_last.bool(), shifted, plain))
        self._step, self._offset = s + 1, (self._offset + 1) & _MASK64
        self._state.copy_(torch.tensor([_signed64(self._offset), self._step], dtype=torch.int64))

    # ---- run ------------------------------------------------------------------------------------
    def run(self, n_steps, backend="graph"):
        check_run_steps(n_steps, self.steps_per_graph, backend)
        if not self._primed:
            raise RuntimeError("call reset(x0) before run()")
        n = int(n_steps)
        self._eval_check_run(n, backend)
        if self._i + n > self._cap:
            if self.disturbance is not None:
                raise ValueError(f"{self._i + n} steps since reset, but disturbance has "
                                 f"{self.disturbance.shape[0]} rows")
            self._rebase(max(n, _MIN_LOG_ROWS), carry=True)
        i0 = self._i
        dev = self.model.device
        if n == 0:
            pass
        elif backend == "graph":
            if self._graph is None:
                self._graph = self._capture()
            for _ in range(n // self.steps_per_graph):
                self._graph.replay()
        elif backend == "launches":
            stream = torch.cuda.current_stream(dev)
            step = self._eager.get(stream.cuda_stream)
            if step is None:
                step = self._eager[stream.cuda_stream] = self._make_step(stream)
            for _ in range(n):
                step()
        else:
            self.reference_trace = []
            for i in range(i0, i0 + n):
                self._reference_step(i)
        if backend != "reference":   # the device advanced itself; the host's mirror follows
            self._step += n
            self._offset = (self._offset + n) & _MASK64
        self._i = i0 + n
        x_log, u_log, info_log = self._logs
        return x_log[i0:i0 + n + 1].clone(), u_log[i0:i0 + n].clone(), info_log[i0:i0 + n].clone()


# ---- a batch of loops in lockstep ------------------------------------------------------------------
def check_batch_shapes(nominal_path, disturbance, n_problems: int, nx: int):
    """The batch's per-problem inputs against ``n_problems`` (host only: dtypes and shapes, no
    device is looked at).  Returns ``(O, P)``."""
    B = int(n_problems)
    if B < 1:
        raise ValueError(f"n_problems={n_problems} must be at least 1")
    t = nominal_path
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() not in (3, 4) or \
            t.shape[-1] != 2:
        raise ValueError("nominal_path must be a float64 [B, O, P, 2] or [O, P, 2] tensor")
    if t.dim() == 4 and t.shape[0] != B:
        raise ValueError(f"nominal_path holds {t.shape[0]} problems, n_problems={B}")
    O, P = t.shape[-3], t.shape[-2]
    if O < 1 or P < 1:
        raise ValueError("nominal_path needs at least one obstacle and one row")
    d = disturbance
    if d is not None:
        if not isinstance(d, torch.Tensor) or d.dtype != torch.float64 or d.dim() != 3 or \
                d.shape[1] < 1 or d.shape[2] != nx:
            raise ValueError(f"disturbance must be a float64 [B, D, {nx}] tensor with D >= 1")
        if d.shape[0] != B:
            raise ValueError(f"disturbance holds {d.shape[0]} problems, n_problems={B}")
    return O, P


def batch_x0(x0, n_problems: int, nx: int) -> torch.Tensor:
    """``x0`` of ``reset`` as float64 ``[B, nx]``: given per problem, or ``[nx]`` for all (host
    only)."""
    x0 = torch.as_tensor(x0, dtype=torch.float64)
    if tuple(x0.shape) == (nx,):
        x0 = x0.expand(int(n_problems), nx)
    if tuple(x0.shape) != (int(n_problems), nx):
        raise ValueError(f"x0 must have shape ({nx},) or (n_problems={n_problems}, {nx}), got "
                         f"{tuple(x0.shape)}")
    return x0


class RecedingHorizonBatch(_Evaluated, _Linearized):
    """``n_problems`` receding-horizon loops that advance in lockstep: three launches per control
    step for any B.

    ``nominal_path`` is ``[B, O, P, 2]`` (one obstacle scenario per problem) or ``[O, P, 2]`` (the
    same in every problem); either way it is materialised once as a contiguous ``[B O, P, 2]``.
    ``x_ref_path [P, nx]`` and ``u_ref_path [P, nu]`` are shared by all problems, or per problem
    (below); ``disturbance`` is ``[B, D, nx]`` or None.  The other arguments are
    :class:`RecedingHorizonFilter`'s.  One control step is

    1. one ``drcvar_sampled_halfspaces_f64_dev`` launch over the B O obstacles (``T = H``), writing
       the record ``[B O, H, 8]``;
    2. one ``filter_batch`` of B problems on ``record.view(B, O, H, 8)`` (strided views, no copy);
    3. one ``drcvar_mpc_step_advance_batch_f64`` launch, one workgroup and one 16-byte state per
       problem.  All B states are kept equal; the halfspace launch reads ``state[0]``.

    Draws: problem b, obstacle o, window step t is unit ``(b O + o) H + t`` of the halfspace launch,
    so the problems get independent draws from the one ``seed`` and stream offset, and with B = 1
    the loop is :class:`RecedingHorizonFilter`'s, bit for bit.  With ``linearize="reference"`` the
    records do not depend on ``metric``: batches built with the same seed, offset and paths see
    the same halfspace records at equal steps, so mean, CVaR and DR-CVaR can be compared on common
    random numbers by running three batches, or as one batch with a metric per problem (below).  With
    ``linearize="predicted"`` (:class:`RecedingHorizonFilter`; step 1 is then
    ``drcvar_sampled_halfspaces_f64_pred`` on ``x0 [B, nx]`` and ``x_out [B, H + 1, nx]``, and
    problems that differ in ``x0`` or disturbance get different halfspaces) the records follow each
    loop's own motion and therefore its metric; the DRAWS are still common random numbers across
    batches with the same seed and offset.

    ``params=engine.RiskTable(...)`` (B rows) gives every loop its own (alpha, delta, epsilon):
    step 1 is then one ``drcvar_sampled_halfspaces_f64_risk`` launch (``include/drcvar_loop_risk.h``,
    DESIGN.md §5.7) whose unit reads its problem's row of the table, and ``draw_period=D`` (None:
    B) makes problem b draw unit ``((b mod D) O + o) H + t``: with B = S D and ``b = s D + r``, S
    settings meet the same D replicate draws in one batch (common random numbers), D = 1 gives every
    problem the same draws.  The solve, the advance and the evaluation launch are untouched, the
    radii stay scalars (``LoopEvaluation`` has scalar radii), and the ``reference`` backend calls
    ``engine.sampled_halfspaces`` per problem with ``params.row(b)``.  A ``RiskTable`` with
    ``linearize="predicted"``, one whose length is not B, or a ``draw_period`` beside a
    ``RiskParams`` is a ``ValueError``; with a ``RiskParams`` the batch is what it was.

    ``metric`` may be a sequence of B names: every loop then filters under its OWN metric
    (``metrics`` holds the B names; with a string it is that name B times).  Step 1 is one
    ``drcvar_sampled_halfspaces_f64_metric`` launch (``include/drcvar_loop_metric.h``, DESIGN.md
    §5.8): the risk-table launch, whose storing lane also writes the unit's chosen ``(h0, h1, g,
    0)`` into ``[B O, H, 4]``; step 2 solves on ``engine.selected_views`` of that.  ``params`` may
    then be a ``RiskTable`` or a ``RiskParams`` (taken as a table of B equal rows; ``params`` then
    holds that table), ``draw_period`` is allowed with either, and S metrics x D replicates with
    ``b = s D + r`` and ``draw_period=D`` is the three-metric comparison on common random numbers
    as one batch.  The ``reference`` backend gathers each problem's columns from the per-problem
    records with torch indexing.  A sequence whose length is not B, an unknown name, or a sequence
    with ``linearize="predicted"`` is a ``ValueError``; with a string the batch is what it was,
    launch for launch.

    ``x_ref_path`` may be ``[B, P, nx]`` and ``u_ref_path`` ``[B, P, nu]``: every loop then follows
    its OWN route (``include/drcvar_loop_route.h``).  If either is 3-D both are
    materialised as contiguous ``[B, P, .]`` and ``ego_path`` is ``[B, P, 2]``.  With
    ``linearize="reference"`` step 1 is one ``drcvar_sampled_halfspaces_f64_route`` launch, the
    metric launch whose unit takes its ego row from its own problem's path: a ``RiskParams`` is
    taken as a table of B equal rows and a string metric as B equal codes, ``draw_period`` (None:
    B) is allowed, and step 2 solves on ``engine.selected_views``.  With
    ``linearize="predicted"`` step 1 stays the ``_pred`` launch, which reads no ego path.  Step 3
    is ``drcvar_mpc_step_advance_batch_route_f64`` either way: workgroup b refills ``x_ref_win[b]``
    and ``u_fallback[b]`` from problem b's paths.  ``reset`` and the ``reference`` backend gather
    each problem's own windows (``engine.sampled_halfspaces`` per problem on that problem's ego
    window; the advance in torch ops with a per-problem ``index_select``).  A 3-D path whose first
    dimension is not B is a ``ValueError``; with 2-D paths the batch is what it was, launch for
    launch, and the route library is not loaded.

    ``noise=engine.NoiseTable(...)`` gives every obstacle and look-ahead step its own noise factor
    (``include/drcvar_loop_noise.h``): ``chol`` is ``[H, 3]``, ``[O, H, 3]`` or
    ``[B, O, H, 3]`` with H the model's horizon.  Step 1 is then one
    ``drcvar_sampled_halfspaces_f64_noise`` launch, the route launch whose unit ``(o, t)`` reads its
    factor from row ``(o mod period) H + t`` of a table on the device; a ``RiskParams`` and a string
    metric are promoted as routes promote them, 2-D paths run with problem stride 0, and the solve,
    both advance kernels and the evaluation launch are untouched.  ``noise_cov`` and ``chol`` are
    then not read by the halfspaces and must be left at their defaults; ``LoopEvaluation`` keeps
    its own covariance, so an assumed schedule can be held against a true noise.  The ``reference``
    backend makes one ``engine.sampled_halfspaces(..., chol=f)`` call per problem and distinct
    factor and takes the units that carry ``f``.  A table whose H or leading dimensions do not
    match, ``noise`` with ``linearize="predicted"`` or beside a ``noise_cov`` / ``chol`` is a
    ``ValueError``; with ``noise=None`` the batch is what it was, launch for launch, and the noise
    library is not loaded.

    ``reset(x0)`` takes ``[B, nx]`` or ``[nx]``.  ``run(n, backend)`` returns ``(states [B, n + 1,
    nx], inputs [B, n, nu], info [B, n, 10])``; backends, log capacity, rebasing, the limit of D
    steps per reset under a disturbance and the treatment of failed solves (a logged step; nothing
    synchronises or retries) are the single class's.  The ``reference`` backend solves all B
    problems in one ``filter_batch`` call (the solver's workgroup size depends on B, so a problem
    solved alone need not be bitwise the problem solved in the batch).
    """

    def __init__(self, model: MPCModel, nominal_path, x_ref_path, u_ref_path, n_samples, params, *,
                 n_problems, metric="dr_cvar", noise_cov=DEFAULT_NOISE_COV, chol=None, seed=0,
                 zero_first_step=True, max_iter=DEFAULT_MAX_ITER, tol=DEFAULT_TOL, polish=True,
                 options=None, disturbance=None, steps_per_graph=1, evaluate=None,
                 linearize="reference", relinearize=0, draw_period=None, noise=None):
        names = check_metric(metric, n_problems, linearize)
        if int(steps_per_graph) < 1:
            raise ValueError(f"steps_per_graph={steps_per_graph} must be at least 1")
        check_evaluate(evaluate)
        check_linearize(linearize, relinearize)
        if noise is not None:   # a noise factor per obstacle and look-ahead step
            if not isinstance(noise, engine.NoiseTable):
                raise ValueError("noise must be an engine.NoiseTable or None")
            if linearize == "predicted":
                raise ValueError('a NoiseTable cannot be combined with linearize="predicted"')
            if chol is not None or noise_cov is not DEFAULT_NOISE_COV:
                raise ValueError("with noise= the halfspaces ignore noise_cov and chol: leave them "
                                 "at their defaults")
            noise.validate()
            if noise.horizon != model.horizon:
                raise ValueError(f"the NoiseTable has H={noise.horizon}, the model's horizon is "
                                 f"{model.horizon}")
        # a route per problem: either reference path is [B, P, .]
        routes = any(isinstance(t, torch.Tensor) and t.dim() == 3 for t in (x_ref_path, u_ref_path))
        if (routes or noise is not None) and names is None and linearize == "reference":
            # the route launch (and the noise launch, a route launch) is a metric launch: B equal codes
            if int(n_problems) < 1:
                raise ValueError(f"n_problems={n_problems} must be at least 1")
            names = (metric,) * int(n_problems)
        if names is not None and not isinstance(params, engine.RiskTable):
            # a metric per problem rides on the risk-table launch: B equal rows
            params.validate()
            params = engine.RiskTable(alpha=[params.alpha] * len(names), delta=params.delta,
                                      epsilon=params.epsilon, robot_radius=params.robot_radius,
                                      obstacle_radius=params.obstacle_radius)
        self.draw_period = check_risk(params, draw_period, n_problems, linearize)
        n = int(n_samples)
        if n < 1 or n > _native.MAX_SAMPLES:
            raise ValueError(f"n_samples={n} outside 1..{_native.MAX_SAMPLES}")
        params.validate()
        dev = model.device
        H, nx, nu = model.horizon, model.nx, model.nu
        B = int(n_problems)
        O, P = check_batch_shapes(nominal_path, disturbance, B, nx)
        self.noise = noise
        self._noise_period = None if noise is None else noise.period(B, O)
        paths = ((x_ref_path, "x_ref_path", nx), (u_ref_path, "u_ref_path", nu))
        for t, name, _ in paths:   # (both, before either's device is looked at)
            if isinstance(t, torch.Tensor) and t.dim() == 3 and t.shape[0] != B:
                raise ValueError(f"{name} holds {t.shape[0]} problems, n_problems={B}")
        for t, name, width in paths:
            per_problem = isinstance(t, torch.Tensor) and t.dim() == 3
            engine.check_path(t, name, (B, P, width) if per_problem else (P, width))
        for t, name in ((nominal_path, "nominal_path"), (x_ref_path, "x_ref_path"),
                        (u_ref_path, "u_ref_path"), (disturbance, "disturbance")):
            if t is not None and t.device != dev:
                raise ValueError(f"{name} must live on the model's device {dev}, got {t.device}")
        self.model, self.params, self.metric = model, params, metric
        self.metrics = names if names is not None else (metric,) * B
        self.n_problems, self.n_obstacles = B, O
        self.n_samples, self.seed = n, int(seed) & _MASK64
        self.noise_cov, self.chol, self.zero_first_step = noise_cov, chol, bool(zero_first_step)
        self.max_iter, self.tol, self.polish, self.options = int(max_iter), float(tol), bool(polish), options
        self.steps_per_graph = int(steps_per_graph)
        self.nominal_path = nominal_path.expand(B, O, P, 2).reshape(B * O, P, 2).contiguous()
        self.routes = routes
        if routes:   # both paths [B, P, .], whichever was given per problem
            x_ref_path, u_ref_path = x_ref_path.expand(B, P, nx), u_ref_path.expand(B, P, nu)
        self.x_ref_path = x_ref_path.contiguous()
        self.u_ref_path = u_ref_path.contiguous()
        self.disturbance = None if disturbance is None else disturbance.contiguous()
        self.path_steps = P
        C = torch.as_tensor(model.C).to(dev)
        if routes:   # [B, P, 2]: per problem the product the shared path takes, so equal routes
            #          give the shared path's bits
            self.ego_path = torch.stack([(xr @ C.T).contiguous() for xr in self.x_ref_path])
        else:
            self.ego_path = (self.x_ref_path @ C.T).contiguous()   # formed once
        f64 = dict(dtype=torch.float64, device=dev)
        # the fixed buffers every captured launch reads or writes
        self._state = torch.zeros((B, 2), dtype=torch.int64, device=dev)   # B x [stream_offset, step]
        self._x0 = torch.zeros((B, nx), **f64)
        self._x_ref_win = torch.zeros((B, H + 1, nx), **f64)
        self._u_fb = torch.zeros((B, H, nu), **f64)
        self._last_u = torch.zeros((B, H, nu), **f64)
        self._have_last = torch.zeros(B, dtype=torch.int32, device=dev)
        self._record = torch.zeros((B * O, H, engine.OUT_WIDTH), **f64)
        self._x = torch.zeros((B, H + 1, nx), **f64)
        self._u = torch.zeros((B, H, nu), **f64)
        self._info = torch.zeros((B, _native.MPC_INFO_WIDTH), **f64)
        self._workspace = torch.empty(max(model.workspace_doubles(B, O), 1), **f64)
        self._rows = {k: torch.arange(k, device=dev) for k in (H, H + 1)}
        self._eval_init(evaluate, B, O, self.nominal_path)
        self._lin_init(linearize, relinearize, B, O, self.nominal_path)
        # a RiskTable: filled for n_samples and copied to the device once
        self._risk_table = params.to_device(n, dev) if self.draw_period is not None else None
        # a metric per problem: the codes on the device, and what the solve reads in place of
        # record columns
        self._codes = self._selected = None
        if names is not None:
            self._codes = engine.metric_codes(names, B, dev)
            self._selected = torch.zeros((B * O, H, engine.SELECTED_WIDTH), **f64)
        # a NoiseTable: its rows on the device, copied once (without one the library is not loaded)
        self._noise_rows = noise.to_device(dev) if noise is not None else None
        self._logs = None           # (x_log [B, cap + 1, nx], u_log [B, cap, nu], info_log [B, cap, 10])
        self._cap, self._step_begin = 0, 0
        self._primed = False
        self._graph = None
        self._eager = {}
        self.reference_trace = []

    def _views(self, record):
        """(h [B, O, H, 2], g [B, O, H]) strided views of a ``[B O, H, 8]`` record."""
        ch, cg = METRIC_COLUMNS[self.metric]
        r = record.view(self.n_problems, self.n_obstacles, self.model.horizon, engine.OUT_WIDTH)
        return r[..., ch:ch + 2], r[..., cg]

    # ---- priming (torch ops, not a mode of the advance kernel) --------------------------------
    def _window(self, path, first, rows):
        """``[rows, .]`` of a shared path, ``[B, rows, .]`` of per-problem paths."""
        idx = (self._rows[rows] + first).clamp_(0, self.path_steps - 1)
        return path.index_select(path.dim() - 2, idx)

    def _write_state(self):
        word = torch.tensor([_signed64(self._offset), self._step], dtype=torch.int64)
        self._state.copy_(word.expand(self.n_problems, 2))

    def reset(self, x0, step=0, stream_offset=0):
        """Start all B loops at path row ``step`` from the states ``x0`` (``[B, nx]``, or ``[nx]``
        for all) with the stream offset of their first draw; all B device states are filled
        identically."""
        H = self.model.horizon
        if self.evaluate is not None:
            check_evaluated_steps(int(step), int(step), self._noise_steps)
        x0 = batch_x0(x0, self.n_problems, self.model.nx).to(self.model.device)
        self._step, self._offset = int(step), int(stream_offset) & _MASK64
        self._write_state()
        self._x0.copy_(x0)
        self._x_ref_win.copy_(self._window(self.x_ref_path, self._step, H + 1))
        self._u_fb.copy_(self._window(self.u_ref_path, self._step, H))
        self._last_u.zero_()
        self._have_last.zero_()
        self._lin_prime()
        self._primed = True
        cap = max(self._cap, _MIN_LOG_ROWS) if self.disturbance is None else self.disturbance.shape[1]
        if self._logs is not None and cap == self._cap and self._step == self._step_begin:
            # the same first step and logs: what was captured stays valid
            for log in self._logs:
                log.fill_(float("nan"))
            self._logs[0][:, 0].copy_(self._x0)
            self._i = 0
        else:
            self._rebase(cap)
        self._eval_reset()

    def _rebase(self, cap, carry=False):
        """New logs of ``cap`` rows per problem whose row 0 is the current step (captured launches
        freeze the log pointers, the row count and the first step, so they are dropped)."""
        self._eval_rebase(cap, carry)
        B, nx, nu = self.n_problems, self.model.nx, self.model.nu
        f64 = dict(dtype=torch.float64, device=self.model.device)
        nan = float("nan")
        self._logs = (torch.full((B, cap + 1, nx), nan, **f64), torch.full((B, cap, nu), nan, **f64),
                      torch.full((B, cap, _native.MPC_INFO_WIDTH), nan, **f64))
        self._logs[0][:, 0].copy_(self._x0)
        self._cap, self._i, self._step_begin = cap, 0, self._step
        self._graph = None
        self._eager = {}

    # ---- one control step as three launches on `stream` -----------------------------------------
    def _make_step(self, stream):
        m = self.model
        H = m.horizon
        again = None
        if self.linearize == "predicted":
            halfspaces = self._lin_launch(stream, 1)
            again = self._lin_launch(stream, 0) if self.relinearize else None
        elif self.noise is not None:
            # the route launch with each unit's own factor; 2-D paths run with problem stride 0
            ego = self.ego_path if self.routes else \
                self.ego_path.expand(self.n_problems, self.path_steps, 2)
            halfspaces, _, _ = engine.prepare_sampled_halfspaces_noise(
                self.nominal_path, ego, self.n_obstacles, H, self.n_samples, self.params,
                self.metrics, self._state[0], self.noise, noise_table=self._noise_rows,
                draw_period=self.draw_period, table=self._risk_table, codes=self._codes,
                seed=self.seed, zero_first_step=self.zero_first_step, out=self._record,
                selected=self._selected, stream=stream)
        elif self._codes is not None:
            prepare = engine.prepare_sampled_halfspaces_route if self.routes else \
                engine.prepare_sampled_halfspaces_metric
            halfspaces, _, _ = prepare(
                self.nominal_path, self.ego_path, self.n_obstacles, H, self.n_samples, self.params,
                self.metrics, self._state[0], draw_period=self.draw_period, table=self._risk_table,
                codes=self._codes, noise_cov=self.noise_cov, seed=self.seed,
                zero_first_step=self.zero_first_step, out=self._record, selected=self._selected,
                stream=stream, chol=self.chol)
        elif self._risk_table is not None:
            halfspaces, _ = engine.prepare_sampled_halfspaces_risk(
                self.nominal_path, self.ego_path, self.n_obstacles, H, self.n_samples, self.params,
                self._state[0], draw_period=self.draw_period, table=self._risk_table,
                noise_cov=self.noise_cov, seed=self.seed, zero_first_step=self.zero_first_step,
                out=self._record, stream=stream, chol=self.chol)
        else:
            halfspaces, _ = engine.prepare_sampled_halfspaces_dev(
                self.nominal_path, self.ego_path, H, self.n_samples, self.params, self._state[0],
                noise_cov=self.noise_cov, seed=self.seed, zero_first_step=self.zero_first_step,
                out=self._record, stream=stream, chol=self.chol)
        if self._codes is not None:
            hs_h, hs_g = engine.selected_views(self._selected, self.n_problems, self.n_obstacles)
        else:
            hs_h, hs_g = self._views(self._record)
        vp = ctypes.c_void_p
        x_log, u_log, info_log = self._logs
        dist = self.disturbance
        if self.routes:   # each problem's own paths: their strides after path_steps
            entry = _native.route_lib().drcvar_mpc_step_advance_batch_route_f64
            strides = (self.x_ref_path.stride(0), self.u_ref_path.stride(0))
        else:
            entry, strides = _native.loop_lib().drcvar_mpc_step_advance_batch_f64, ()
        advance = engine.PreparedLaunch(entry, (
            ctypes.pointer(m.model), self.n_problems, vp(self._x.data_ptr()), vp(self._u.data_ptr()),
            vp(self._info.data_ptr()), vp(self.x_ref_path.data_ptr()), vp(self.u_ref_path.data_ptr()),
            self.path_steps, *strides, vp(dist.data_ptr() if dist is not None else None),
            self._step_begin, self._cap, vp(x_log.data_ptr()), vp(u_log.data_ptr()), vp(info_log.data_ptr()),
            vp(self._x0.data_ptr()), vp(self._x_ref_win.data_ptr()), vp(self._u_fb.data_ptr()),
            vp(self._last_u.data_ptr()), vp(self._have_last.data_ptr()), vp(self._state.data_ptr()),
            vp(int(stream.cuda_stream))), (self, x_log, u_log, info_log))
        out = (self._x, self._u, self._info)
        # with an evaluation: a fourth launch on the same stream, after the advance (x0 is then the
        # state just reached and state.step its path row); the chain stays linear
        evaluation = self._eval_launch(stream) if self.evaluate is not None else None

        def solve():
            filter_batch(m, hs_h, hs_g, self._x0, self._x_ref_win, self._u_fb, self.max_iter,
                         self.tol, self.polish, workspace=self._workspace, stream=stream,
                         options=self.options, out=out)

        def step():
            halfspaces()
            solve()
            # relinearize: the same draws (the state moves only in the advance) about the answer
            # just written, then the solve again; still one linear chain
            for _ in range(self.relinearize):
                again()
                solve()
            advance()
            if evaluation is not None:
                evaluation()
        return step

    def _mutable(self):
        evaluated = [] if self.evaluate is None else [self._min_d2, self._eval_hits]
        # (under "predicted" x_out is an input of the next step's halfspaces)
        predicted = [self._x] if self.linearize == "predicted" else []
        return [self._state, self._x0, self._x_ref_win, self._u_fb, self._last_u, self._have_last,
                *self._logs, *evaluated, *predicted]

    # ---- the semantics, from the entry points that predate the loop -----------------------------
    def _risk_reference_record(self, window, ego_window):
        """The record ``[B O, H, 8]`` of a RiskTable batch from the entry that predates the table:
        per problem one ``engine.sampled_halfspaces`` call with ``params.row(b)`` on a nominal
        tensor whose obstacle rows ``(b mod D) O .. + O`` are the problem's gathered window (the
        rows before them are never read) and the unit window that starts there; ``ego_window`` is
        ``[H, 2]``, or ``[B, H, 2]`` with a route per problem."""
        H, B, O, D = self.model.horizon, self.n_problems, self.n_obstacles, self.draw_period
        records = []
        for b in range(B):
            r = b % D
            nominal = torch.zeros(((r + 1) * O, H, 2), dtype=torch.float64, device=window.device)
            nominal[r * O:].copy_(window[b * O:(b + 1) * O])
            records.append(engine.sampled_halfspaces(
                nominal, ego_window[b] if ego_window.dim() == 3 else ego_window, self.n_samples,
                self.params.row(b), noise_cov=self.noise_cov,
                chol=self.chol, seed=self.seed, stream_offset=self._offset,
                zero_first_step=self.zero_first_step, unit_begin=r * O * H, unit_count=O * H))
        return torch.cat(records).view(B * O, H, engine.OUT_WIDTH)

    def _noise_reference_record(self, window, ego_window):
        """The record ``[B O, H, 8]`` of a NoiseTable batch from the entry that predates the table:
        :meth:`_risk_reference_record`'s call once per problem and distinct factor ``f`` of that
        problem's units, with ``chol=f``, from which the units that carry ``f`` are taken."""
        H, B, O, D = self.model.horizon, self.n_problems, self.n_obstacles, self.draw_period
        records = []
        for b in range(B):
            r = b % D
            nominal = torch.zeros(((r + 1) * O, H, 2), dtype=torch.float64, device=window.device)
            nominal[r * O:].copy_(window[b * O:(b + 1) * O])
            carriers = {}
            for o in range(O):
                for t in range(H):
                    carriers.setdefault(self.noise.factor(b * O + o, t), []).append(o * H + t)
            record = torch.empty((O * H, engine.OUT_WIDTH), dtype=torch.float64, device=window.device)
            for f, units in carriers.items():
                part = engine.sampled_halfspaces(
                    nominal, ego_window[b] if ego_window.dim() == 3 else ego_window, self.n_samples,
                    self.params.row(b), chol=f, seed=self.seed, stream_offset=self._offset,
                    zero_first_step=self.zero_first_step, unit_begin=r * O * H, unit_count=O * H)
                idx = torch.tensor(units, device=window.device)
                record[idx] = part[idx]
            records.append(record)
        return torch.cat(records).view(B * O, H, engine.OUT_WIDTH)

    def _reference_selected(self, record):
        """``[B O, H, 4]``: each problem's ``METRIC_COLUMNS`` gathered from ``record`` with torch
        indexing, the fourth column zero (what the metric launch stores beside the record)."""
        B, O = self.n_problems, self.n_obstacles
        cols = torch.tensor([[c, c + 1, g] for c, g in (METRIC_COLUMNS[m] for m in self.metrics)],
                            device=record.device).repeat_interleave(O, dim=0)      # [B O, 3]
        selected = torch.zeros((B * O, record.shape[1], engine.SELECTED_WIDTH), dtype=record.dtype,
                               device=record.device)
        selected[..., :3] = record.gather(2, cols[:, None, :].expand(-1, record.shape[1], -1))
        return selected

    def _reference_step(self, i):
        m = self.model
        H, B = m.horizon, self.n_problems
        s = self._step
        window = self.nominal_path.index_select(
            1, (self._rows[H] + s).clamp_(0, self.path_steps - 1))     # [B O, H, 2]
        for p in range(1 + self.relinearize):
            if self.linearize == "predicted":
                record = self._lin_reference_record(window, 1 if p == 0 else 0)
            elif self.noise is not None:
                record = self._noise_reference_record(window, self._window(self.ego_path, s, H))
            elif self._risk_table is not None:
                record = self._risk_reference_record(window, self._window(self.ego_path, s, H))
            else:
                ego_window = self._window(self.ego_path, s, H)
                record = engine.sampled_halfspaces(window, ego_window, self.n_samples, self.params,
                                                   noise_cov=self.noise_cov, chol=self.chol,
                                                   seed=self.seed, stream_offset=self._offset,
                                                   zero_first_step=self.zero_first_step)
            if self._codes is not None:
                hs_h, hs_g = engine.selected_views(self._reference_selected(record), B,
                                                   self.n_obstacles)
            else:
                hs_h, hs_g = self._views(record)
            x, u, info = filter_batch(m, hs_h, hs_g, self._x0, self._x_ref_win, self._u_fb,
                                      self.max_iter, self.tol, self.polish, options=self.options)
            self._x.copy_(x)   # (the next linearisation point; the device backends' x_out)
        self.reference_trace.append((x.clone(), u.clone(), info.clone()))
        x_log, u_log, info_log = self._logs
        x_next = x[:, 1]
        if self.disturbance is not None:
            x_next = x_next + self.disturbance[:, i]
        x_log[:, i + 1].copy_(x_next)
        u_log[:, i].copy_(u[:, 0])
        info_log[:, i].copy_(info)
        status = info[:, _native.MPC_INFO_STATUS]
        solved = (status == _native.MPC_STATUS_OPTIMAL) | (status == _native.MPC_STATUS_OPTIMAL_INACCURATE)
        self._last_u.copy_(torch.where(solved[:, None, None], u, self._last_u))
        self._have_last.copy_(torch.where(solved, torch.ones_like(self._have_last), self._have_last))
        self._x0.copy_(x_next)
        self._x_ref_win.copy_(self._window(self.x_ref_path, s + 1, H + 1))
        plain = self._window(self.u_ref_path, s + 1, H)
        shifted = torch.cat((self._last_u[:, 1:], plain[..., H - 1:, :].expand(B, 1, m.nu)), dim=1)
        self._u_fb.copy_(torch.where(self._have_last.bool()[:, None, None], shifted, plain))
        self._step, self._offset = s + 1, (self._offset + 1) & _MASK64
        self._write_state()

    # ---- run ------------------------------------------------------------------------------------
    def run(self, n_steps, backend="graph"):
        check_run_steps(n_steps, self.steps_per_graph, backend)
        if not self._primed:
            raise RuntimeError("call reset(x0) before run()")
        n = int(n_steps)
        self._eval_check_run(n, backend)
        if self._i + n > self._cap:
            if self.disturbance is not None:
                raise ValueError(f"{self._i + n} steps since reset, but disturbance has "
                                 f"{self.disturbance.shape[1]} rows")
            self._rebase(max(n, _MIN_LOG_ROWS), carry=True)
        i0 = self._i
        dev = self.model.device
        if n == 0:
            pass
        elif backend == "graph":
            if self._graph is None:
                self._graph = _capture_chain(dev, self._make_step, self._mutable, self.steps_per_graph)
            for _ in range(n // self.steps_per_graph):
                self._graph.replay()
        elif backend == "launches":
            stream = torch.cuda.current_stream(dev)
            step = self._eager.get(stream.cuda_stream)
            if step is None:
                step = self._eager[stream.cuda_stream] = self._make_step(stream)
            for _ in range(n):
                step()
        else:
            self.reference_trace = []
            for i in range(i0, i0 + n):
                self._reference_step(i)
        if backend != "reference":   # the device advanced itself; the host's mirror follows
            self._step += n
            self._offset = (self._offset + n) & _MASK64
        self._i = i0 + n
        x_log, u_log, info_log = self._logs
        return (x_log[:, i0:i0 + n + 1].clone(), u_log[:, i0:i0 + n].clone(),
                info_log[:, i0:i0 + n].clone())
