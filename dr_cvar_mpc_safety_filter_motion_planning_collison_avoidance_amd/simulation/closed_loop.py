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

The halfspaces are computed about the REFERENCE path (``ego_path = x_ref_path @ C.T``), as the
reference does (``main.py:95-97``), not about the actual state.  One problem per loop;
:class:`RecedingHorizonBatch` advances B loops in lockstep with the same three launches per step
(``drcvar_mpc_step_advance_batch_f64``, ``include/drcvar_loop.h``: one workgroup and one device state per problem, DESIGN.md
§5.4).
"""
from __future__ import annotations

import ctypes

import torch

from .. import _native, engine
from ..core.mpc_filter import (DEFAULT_MAX_ITER, DEFAULT_TOL, METRIC_COLUMNS, MPCModel, filter_batch,
                               record_views)
from ..engine import DEFAULT_NOISE_COV

BACKENDS = ("graph", "launches", "reference")
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


class RecedingHorizonFilter:
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
    """

    def __init__(self, model: MPCModel, nominal_path, x_ref_path, u_ref_path, n_samples, params, *,
                 metric="dr_cvar", noise_cov=DEFAULT_NOISE_COV, chol=None, seed=0,
                 zero_first_step=True, max_iter=DEFAULT_MAX_ITER, tol=DEFAULT_TOL, polish=True,
                 options=None, disturbance=None, steps_per_graph=1):
        if metric not in METRIC_COLUMNS:
            raise ValueError(f"metric must be one of {tuple(METRIC_COLUMNS)}, got {metric!r}")
        if int(steps_per_graph) < 1:
            raise ValueError(f"steps_per_graph={steps_per_graph} must be at least 1")
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
        x0 = torch.as_tensor(x0, dtype=torch.float64).reshape(1, self.model.nx).to(dev)
        self._step, self._offset = int(step), int(stream_offset) & _MASK64
        self._state.copy_(torch.tensor([_signed64(self._offset), self._step], dtype=torch.int64))
        self._x0.copy_(x0)
        self._x_ref_win[0].copy_(self._window(self.x_ref_path, self._step, H + 1))
        self._u_fb[0].copy_(self._window(self.u_ref_path, self._step, H))
        self._last_u.zero_()
        self._have_last.zero_()
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

    def _rebase(self, cap):
        """New logs of ``cap`` rows whose row 0 is the current step (captured launches freeze the
        log pointers and the first step, so they are dropped)."""
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

        def step():
            halfspaces()
            filter_batch(m, hs_h, hs_g, self._x0, self._x_ref_win, self._u_fb, self.max_iter,
                         self.tol, self.polish, workspace=self._workspace, stream=stream,
                         options=self.options, out=out)
            advance()
        return step

    def _mutable(self):
        return [self._state, self._x0, self._x_ref_win, self._u_fb, self._last_u, self._have_last,
                *self._logs]

    def _capture(self):
        return _capture_chain(self.model.device, self._make_step, self._mutable, self.steps_per_graph)

    # ---- the semantics, from the entry points that predate the loop -----------------------------
    def _reference_step(self, i):
        m = self.model
        H = m.horizon
        s = self._step
        window = self.nominal_path.index_select(
            1, (self._rows[H] + s).clamp_(0, self.path_steps - 1))
        ego_window = self._window(self.ego_path, s, H)
        record = engine.sampled_halfspaces(window, ego_window, self.n_samples, self.params,
                                           noise_cov=self.noise_cov, chol=self.chol, seed=self.seed,
                                           stream_offset=self._offset,
                                           zero_first_step=self.zero_first_step)
        hs_h, hs_g = record_views(record[:, :H], self.metric)
        x, u, info = filter_batch(m, hs_h, hs_g, self._x0, self._x_ref_win, self._u_fb,
                                  self.max_iter, self.tol, self.polish, options=self.options)
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
        if self._i + n > self._cap:
            if self.disturbance is not None:
                raise ValueError(f"{self._i + n} steps since reset, but disturbance has "
                                 f"{self.disturbance.shape[0]} rows")
            self._rebase(max(n, _MIN_LOG_ROWS))
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


class RecedingHorizonBatch:
    """``n_problems`` receding-horizon loops that advance in lockstep: three launches per control
    step for any B.

    ``nominal_path`` is ``[B, O, P, 2]`` (one obstacle scenario per problem) or ``[O, P, 2]`` (the
    same in every problem); either way it is materialised once as a contiguous ``[B O, P, 2]``.
    ``x_ref_path [P, nx]`` and ``u_ref_path [P, nu]`` are shared by all problems (the halfspace
    launch has one ego path); ``disturbance`` is ``[B, D, nx]`` or None.  The other arguments are
    :class:`RecedingHorizonFilter`'s.  One control step is

    1. one ``drcvar_sampled_halfspaces_f64_dev`` launch over the B O obstacles (``T = H``), writing
       the record ``[B O, H, 8]``;
    2. one ``filter_batch`` of B problems on ``record.view(B, O, H, 8)`` (strided views, no copy);
    3. one ``drcvar_mpc_step_advance_batch_f64`` launch, one workgroup and one 16-byte state per
       problem.  All B states are kept equal; the halfspace launch reads ``state[0]``.

    Draws: problem b, obstacle o, window step t is unit ``(b O + o) H + t`` of the halfspace launch,
    so the problems get independent draws from the one ``seed`` and stream offset, and with B = 1
    the loop is :class:`RecedingHorizonFilter`'s, bit for bit.  The records do not depend on
    ``metric``: batches built with the same seed, offset and paths see the same halfspace records
    at equal states, so mean, CVaR and DR-CVaR are compared on common random numbers by running
    three batches (there is no per-problem metric).

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
                 options=None, disturbance=None, steps_per_graph=1):
        if metric not in METRIC_COLUMNS:
            raise ValueError(f"metric must be one of {tuple(METRIC_COLUMNS)}, got {metric!r}")
        if int(steps_per_graph) < 1:
            raise ValueError(f"steps_per_graph={steps_per_graph} must be at least 1")
        n = int(n_samples)
        if n < 1 or n > _native.MAX_SAMPLES:
            raise ValueError(f"n_samples={n} outside 1..{_native.MAX_SAMPLES}")
        params.validate()
        dev = model.device
        H, nx, nu = model.horizon, model.nx, model.nu
        B = int(n_problems)
        O, P = check_batch_shapes(nominal_path, disturbance, B, nx)
        engine.check_path(x_ref_path, "x_ref_path", (P, nx))
        engine.check_path(u_ref_path, "u_ref_path", (P, nu))
        for t, name in ((nominal_path, "nominal_path"), (x_ref_path, "x_ref_path"),
                        (u_ref_path, "u_ref_path"), (disturbance, "disturbance")):
            if t is not None and t.device != dev:
                raise ValueError(f"{name} must live on the model's device {dev}, got {t.device}")
        self.model, self.params, self.metric = model, params, metric
        self.n_problems, self.n_obstacles = B, O
        self.n_samples, self.seed = n, int(seed) & _MASK64
        self.noise_cov, self.chol, self.zero_first_step = noise_cov, chol, bool(zero_first_step)
        self.max_iter, self.tol, self.polish, self.options = int(max_iter), float(tol), bool(polish), options
        self.steps_per_graph = int(steps_per_graph)
        self.nominal_path = nominal_path.expand(B, O, P, 2).reshape(B * O, P, 2).contiguous()
        self.x_ref_path = x_ref_path.contiguous()
        self.u_ref_path = u_ref_path.contiguous()
        self.disturbance = None if disturbance is None else disturbance.contiguous()
        self.path_steps = P
        C = torch.as_tensor(model.C).to(dev)
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
        idx = (self._rows[rows] + first).clamp_(0, self.path_steps - 1)
        return path.index_select(0, idx)

    def _write_state(self):
        word = torch.tensor([_signed64(self._offset), self._step], dtype=torch.int64)
        self._state.copy_(word.expand(self.n_problems, 2))

    def reset(self, x0, step=0, stream_offset=0):
        """Start all B loops at path row ``step`` from the states ``x0`` (``[B, nx]``, or ``[nx]``
        for all) with the stream offset of their first draw; all B device states are filled
        identically."""
        H = self.model.horizon
        x0 = batch_x0(x0, self.n_problems, self.model.nx).to(self.model.device)
        self._step, self._offset = int(step), int(stream_offset) & _MASK64
        self._write_state()
        self._x0.copy_(x0)
        self._x_ref_win.copy_(self._window(self.x_ref_path, self._step, H + 1))
        self._u_fb.copy_(self._window(self.u_ref_path, self._step, H))
        self._last_u.zero_()
        self._have_last.zero_()
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

    def _rebase(self, cap):
        """New logs of ``cap`` rows per problem whose row 0 is the current step (captured launches
        freeze the log pointers, the row count and the first step, so they are dropped)."""
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
        halfspaces, _ = engine.prepare_sampled_halfspaces_dev(
            self.nominal_path, self.ego_path, H, self.n_samples, self.params, self._state[0],
            noise_cov=self.noise_cov, seed=self.seed, zero_first_step=self.zero_first_step,
            out=self._record, stream=stream, chol=self.chol)
        hs_h, hs_g = self._views(self._record)
        vp = ctypes.c_void_p
        x_log, u_log, info_log = self._logs
        dist = self.disturbance
        advance = engine.PreparedLaunch(_native.loop_lib().drcvar_mpc_step_advance_batch_f64, (
            ctypes.pointer(m.model), self.n_problems, vp(self._x.data_ptr()), vp(self._u.data_ptr()),
            vp(self._info.data_ptr()), vp(self.x_ref_path.data_ptr()), vp(self.u_ref_path.data_ptr()),
            self.path_steps, vp(dist.data_ptr() if dist is not None else None), self._step_begin,
            self._cap, vp(x_log.data_ptr()), vp(u_log.data_ptr()), vp(info_log.data_ptr()),
            vp(self._x0.data_ptr()), vp(self._x_ref_win.data_ptr()), vp(self._u_fb.data_ptr()),
            vp(self._last_u.data_ptr()), vp(self._have_last.data_ptr()), vp(self._state.data_ptr()),
            vp(int(stream.cuda_stream))), (self, x_log, u_log, info_log))
        out = (self._x, self._u, self._info)

        def step():
            halfspaces()
            filter_batch(m, hs_h, hs_g, self._x0, self._x_ref_win, self._u_fb, self.max_iter,
                         self.tol, self.polish, workspace=self._workspace, stream=stream,
                         options=self.options, out=out)
            advance()
        return step

    def _mutable(self):
        return [self._state, self._x0, self._x_ref_win, self._u_fb, self._last_u, self._have_last,
                *self._logs]

    # ---- the semantics, from the entry points that predate the loop -----------------------------
    def _reference_step(self, i):
        m = self.model
        H, B = m.horizon, self.n_problems
        s = self._step
        window = self.nominal_path.index_select(
            1, (self._rows[H] + s).clamp_(0, self.path_steps - 1))     # [B O, H, 2]
        ego_window = self._window(self.ego_path, s, H)
        record = engine.sampled_halfspaces(window, ego_window, self.n_samples, self.params,
                                           noise_cov=self.noise_cov, chol=self.chol, seed=self.seed,
                                           stream_offset=self._offset,
                                           zero_first_step=self.zero_first_step)
        hs_h, hs_g = self._views(record)
        x, u, info = filter_batch(m, hs_h, hs_g, self._x0, self._x_ref_win, self._u_fb,
                                  self.max_iter, self.tol, self.polish, options=self.options)
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
        shifted = torch.cat((self._last_u[:, 1:], plain[H - 1:].expand(B, 1, m.nu)), dim=1)
        self._u_fb.copy_(torch.where(self._have_last.bool()[:, None, None], shifted, plain))
        self._step, self._offset = s + 1, (self._offset + 1) & _MASK64
        self._write_state()

    # ---- run ------------------------------------------------------------------------------------
    def run(self, n_steps, backend="graph"):
        check_run_steps(n_steps, self.steps_per_graph, backend)
        if not self._primed:
            raise RuntimeError("call reset(x0) before run()")
        n = int(n_steps)
        if self._i + n > self._cap:
            if self.disturbance is not None:
                raise ValueError(f"{self._i + n} steps since reset, but disturbance has "
                                 f"{self.disturbance.shape[1]} rows")
            self._rebase(max(n, _MIN_LOG_ROWS))
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
