"""Tensor-level entry points of the HIP engine (device-resident PyTorch-ROCm tensors).

These are the batched calls everything else is built on:

* :func:`safe_halfspaces`   — ``drcvar_safe_halfspaces_f64``: mean / CVaR / DR-CVaR halfspaces for
  every (obstacle, step) of a ``[O, T, N, 2]`` sample tensor (``core/halfspaces.py:196-248`` x the
  horizon loop of ``simulation/environment.py:82-104``).
* :func:`offsets_given_h`   — ``drcvar_offsets_given_h_f64``: ``cvar_halfspace`` /
  ``dr_cvar_halfspace`` for caller-supplied directions (``core/risk_metrics.py:267-338``).
* :func:`sampled_halfspaces` — ``drcvar_sampled_halfspaces_f64``: the same records straight from
  the nominal paths ``[O, T, 2]``, each unit's samples drawn inside the kernel and never stored
  (``simulation/obstacles.py:43-77`` + ``core/halfspaces.py:196-248`` in one launch).
* :func:`sampled_halfspaces_dev` — ``drcvar_sampled_halfspaces_f64_dev``: the same launch with the
  window start and the stream offset read from a device-resident state, for a receding-horizon
  loop replayed from one graph (``simulation/closed_loop.py``).
* :func:`sampled_halfspaces_pred` — ``drcvar_sampled_halfspaces_f64_pred``: that launch for a
  batch of loops, each unit's ego taken from its own problem's state and predicted path.
* :func:`sampled_halfspaces_risk` — ``drcvar_sampled_halfspaces_f64_risk``: that launch for a
  batch of loops, each unit's risk parameters taken from its own problem's row of a
  :class:`RiskTable`, the draws shared between problems by a draw period.
* :func:`sampled_halfspaces_metric` — ``drcvar_sampled_halfspaces_f64_metric``: the risk-table
  launch that also stores every unit's halfspace under its own problem's metric.

All enqueue one kernel on the current HIP stream and return without synchronising.  Inputs must
be float64 CUDA tensors whose two coordinates are adjacent (last stride 1); any other strides are
passed to the kernel as they are (no hidden copies).  :class:`PreparedLaunch` freezes the argument
tuple of a repeated call (bench loops, graph capture) so the per-launch host cost is one ctypes
call.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import torch

from . import _native

OUT_WIDTH = _native.OUT_WIDTH


@dataclass(frozen=True)
class RiskParams:
    """The five scalars the reference threads through every call (``config/parameters.py:11-29``)."""

    robot_radius: float = 0.3
    obstacle_radius: float = 0.3
    alpha: float = 0.2
    delta: float = 0.1
    epsilon: float = 0.15

    def validate(self) -> None:
        vals = (self.robot_radius, self.obstacle_radius, self.alpha, self.delta, self.epsilon)
        if not all(math.isfinite(v) for v in vals):
            raise ValueError(f"risk parameters must be finite: {self}")
        if self.alpha <= 0.0:
            # the reference divides by alpha while building its LPs (risk_metrics.py:105-107,212)
            raise ValueError(f"alpha must be > 0, got {self.alpha}")


def _stream_handle(device: torch.device, stream=None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return int(s.cuda_stream)


def _check_samples(samples: torch.Tensor, ndim: int) -> None:
    if not isinstance(samples, torch.Tensor):
        raise TypeError("samples must be a torch.Tensor")
    if samples.device.type != "cuda":
        raise ValueError("samples must live on the GPU (HIP device tensor); the engine has no CPU path")
    if samples.dtype != torch.float64:
        raise TypeError(f"samples must be float64 (the reference computes in f64), got {samples.dtype}")
    if samples.dim() != ndim or samples.shape[-1] != 2:
        raise ValueError(f"samples must have shape {'[O, T, N, 2]' if ndim == 4 else '[U, N, 2]'}, "
                         f"got {tuple(samples.shape)}")
    if samples.stride(-1) != 1:
        raise ValueError("the two coordinates of a sample must be adjacent (last stride 1)")
    n = samples.shape[-2]
    if n < 1:
        raise ValueError("each unit needs at least one sample")
    if n > _native.MAX_SAMPLES_STREAM:
        raise ValueError(f"n_samples={n} exceeds the engine limit {_native.MAX_SAMPLES_STREAM}")


def _check_pairs(t: torch.Tensor, name: str, rows: int, device: torch.device) -> None:
    if t.device != device or t.dtype != torch.float64:
        raise ValueError(f"{name} must be a float64 tensor on {device}")
    if t.dim() != 2 or t.shape[0] != rows or t.shape[1] != 2 or t.stride(1) != 1:
        raise ValueError(f"{name} must have shape [{rows}, 2] with adjacent coordinates, got "
                         f"{tuple(t.shape)}")


def _check_out(out, shape, device: torch.device, what: str) -> None:
    """A caller-supplied output buffer must be exactly what the kernel writes: the engine writes
    ``prod(shape) * 8`` doubles through the raw pointer, so anything else is an out-of-bounds
    device write (checked before any ABI call)."""
    if not isinstance(out, torch.Tensor):
        raise TypeError("out must be a torch.Tensor")
    if (tuple(out.shape) != tuple(shape) or out.dtype != torch.float64 or not out.is_contiguous()
            or out.device != device):
        raise ValueError(f"out must be a contiguous float64 {what} tensor on {device}, got "
                         f"{tuple(out.shape)} {out.dtype} on {out.device}"
                         f"{'' if out.is_contiguous() else ' (non-contiguous)'}")


def _typed(args):
    """Pre-convert an argument tuple to ctypes objects (saves the per-call conversion)."""
    out = []
    for a in args:
        if isinstance(a, (ctypes._SimpleCData, ctypes._Pointer)):   # (a pointer: a struct argument)
            out.append(a)
        elif isinstance(a, bool) or not isinstance(a, (int, float)):
            raise TypeError(f"unexpected argument {a!r}")
        elif isinstance(a, int):
            out.append(ctypes.c_int64(a))
        else:
            out.append(ctypes.c_double(a))
    return tuple(out)


class PreparedLaunch:
    """A frozen engine call: same buffers, same parameters, relaunched by ``__call__``."""

    def __init__(self, fn, args, keepalive):
        self._fn = fn
        self._args = _typed(args)
        self._keepalive = keepalive  # tensors whose storage the pointers refer to

    def __call__(self) -> None:
        code = self._fn(*self._args)
        if code != _native.OK:
            _native.check(code)


def _check_status(status, n, device):
    if not isinstance(status, torch.Tensor) or status.dtype != torch.int32 or status.device != device \
            or status.numel() != n or not status.is_contiguous():
        raise ValueError(f"status must be a contiguous int32 tensor of {n} elements on {device}")


def prepare_safe_halfspaces(samples: torch.Tensor, ego: torch.Tensor, params: RiskParams,
                            out: torch.Tensor | None = None, stream=None,
                            geometry: tuple[int, int] | None = None,
                            status: torch.Tensor | None = None) -> tuple[PreparedLaunch, torch.Tensor]:
    """Freeze one ``drcvar_safe_halfspaces_f64`` call; ``geometry=(threads, per_thread)`` selects a
    specific compiled launch geometry, ``status`` (int32 ``[O, T]``) receives the per-unit status
    word (``_native.UNIT_*``) — both through ``drcvar_safe_halfspaces_f64_v2``."""
    params.validate()
    _check_samples(samples, 4)
    O, T, N, _ = samples.shape
    _check_pairs(ego, "ego", T, samples.device)
    if out is None:
        out = torch.empty((O, T, OUT_WIDTH), dtype=torch.float64, device=samples.device)
    else:
        _check_out(out, (O, T, OUT_WIDTH), samples.device, "[O, T, 8]")
    lib = _native.lib()
    so, st, sn = samples.stride(0), samples.stride(1), samples.stride(2)
    args = (ctypes.c_void_p(samples.data_ptr()), O, T, N, so, st, sn,
            ctypes.c_void_p(ego.data_ptr()), ego.stride(0),
            params.robot_radius, params.obstacle_radius, params.alpha, params.delta, params.epsilon,
            ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(_stream_handle(samples.device, stream)))
    if geometry is not None or status is not None:
        if status is not None:
            _check_status(status, O * T, samples.device)
        geo = tuple(ctypes.c_int32(int(g)) for g in (geometry or (0, 0)))
        st_ptr = ctypes.c_void_p(status.data_ptr() if status is not None else None)
        args2 = args[:-1] + (st_ptr, args[-1]) + geo
        return PreparedLaunch(lib.drcvar_safe_halfspaces_f64_v2, args2, (samples, ego, out, status)), out
    return PreparedLaunch(lib.drcvar_safe_halfspaces_f64, args, (samples, ego, out)), out


def safe_halfspaces(samples: torch.Tensor, ego: torch.Tensor, params: RiskParams = RiskParams(),
                    out: torch.Tensor | None = None, stream=None,
                    status: torch.Tensor | None = None) -> torch.Tensor:
    """Mean / CVaR / DR-CVaR halfspaces of every (obstacle, step) unit.

    samples [O, T, N, 2] float64 (device), ego [T, 2] float64 (device) -> [O, T, 8] float64 with
    columns (mean_h0, mean_h1, g_mean, h0, h1, g_cvar, g_dr_star, g_dr_tilde).  ``status``
    (optional int32 ``[O, T]`` device tensor) receives each unit's ``_native.UNIT_*`` bits.
    """
    launch, out = prepare_safe_halfspaces(samples, ego, params, out, stream, status=status)
    if samples.shape[0] * samples.shape[1] > 0:
        launch()
    return out


DEFAULT_NOISE_COV = ((0.01, 0.0), (0.0, 0.01))  # the reference's default, simulation/obstacles.py:134


def _noise_factor(noise_cov, chol):
    """(l00, l10, l11): ``chol`` as given (it may be singular or zero), else the lower Cholesky
    factor of ``noise_cov`` exactly as ``sample_trajectories_device`` forms it."""
    if chol is not None:
        l00, l10, l11 = (float(v) for v in chol)
        return l00, l10, l11
    import numpy as np
    L = np.linalg.cholesky(np.asarray(noise_cov, dtype=np.float64).reshape(2, 2))
    return float(L[0, 0]), float(L[1, 0]), float(L[1, 1])


def prepare_sampled_halfspaces(nominal: torch.Tensor, ego: torch.Tensor, n_samples: int,
                               params: RiskParams = RiskParams(), noise_cov=DEFAULT_NOISE_COV,
                               seed: int = 0, stream_offset: int = 0, zero_first_step: bool = True,
                               unit_begin: int = 0, unit_count: int | None = None,
                               out: torch.Tensor | None = None, status: torch.Tensor | None = None,
                               samples_out: torch.Tensor | None = None, stream=None,
                               chol=None) -> tuple[PreparedLaunch, torch.Tensor]:
    """Freeze one ``drcvar_sampled_halfspaces_f64`` call: halfspaces straight from the nominal
    paths, the samples drawn in the kernel and never stored.

    nominal ``[O, T, 2]`` and ego ``[T, 2]`` float64 device tensors with adjacent coordinates;
    ``1 <= n_samples <= _native.MAX_SAMPLES``.  The noise is ``noise_cov`` through
    ``np.linalg.cholesky`` (as ``sample_trajectories_device``), or an explicit lower factor
    ``chol=(l00, l10, l11)``, which may be singular or zero.  With ``unit_count=None`` the whole
    grid is evaluated and ``out`` is ``[O, T, 8]``; a unit window ``[unit_begin, unit_begin +
    unit_count)`` (unit ``u = o * T + t``) gives ``[unit_count, 8]``.  ``status`` (int32, one
    element per unit) receives the ``_native.UNIT_*`` bits; ``samples_out`` (``[units, N, 2]``
    float64 view with adjacent coordinates; ``[O, T, N, 2]`` contiguous in its first two axes for
    the whole grid) also receives the samples drawn — the records are the same bits without it.
    A frozen launch replays the same draw (graph capture included)."""
    params.validate()
    if not isinstance(nominal, torch.Tensor) or nominal.device.type != "cuda":
        raise ValueError("nominal must live on the GPU (HIP device tensor); the engine has no CPU path")
    if nominal.dtype != torch.float64 or nominal.dim() != 3 or nominal.shape[2] != 2 or \
            nominal.stride(2) != 1:
        raise ValueError("nominal must be float64 [O, T, 2] with adjacent coordinates")
    dev = nominal.device
    O, T, _ = nominal.shape
    n = int(n_samples)
    if n < 1 or n > _native.MAX_SAMPLES:
        raise ValueError(f"n_samples={n} outside 1..{_native.MAX_SAMPLES} (the sampled form holds a "
                         "unit on chip; larger units go through the sampler and safe_halfspaces)")
    _check_pairs(ego, "ego", T, dev)
    whole = unit_count is None
    u0 = int(unit_begin)
    count = O * T - u0 if whole else int(unit_count)
    if u0 < 0 or count < 0 or u0 + count > O * T:
        raise ValueError(f"unit range [{u0}, {u0 + count}) outside the {O} x {T} grid")
    whole = whole and u0 == 0
    shape = (O, T, OUT_WIDTH) if whole else (count, OUT_WIDTH)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=dev)
    else:
        _check_out(out, shape, dev, "[O, T, 8]" if whole else "[units, 8]")
    if status is not None:
        _check_status(status, count, dev)
    su = sn = 0
    if samples_out is not None:
        s = samples_out
        if not isinstance(s, torch.Tensor) or s.dtype != torch.float64 or s.device != dev or \
                s.shape[-1] != 2 or s.stride(-1) != 1:
            raise ValueError("samples_out must be a float64 device view with adjacent coordinates")
        if whole and tuple(s.shape) == (O, T, n, 2) and (O <= 1 or s.stride(0) == T * s.stride(1)):
            su, sn = s.stride(1), s.stride(2)
        elif tuple(s.shape) == (count, n, 2):
            su, sn = s.stride(0), s.stride(1)
        else:
            raise ValueError(f"samples_out must have shape {(count, n, 2)}"
                             f"{' or ' + str((O, T, n, 2)) if whole else ''}, got {tuple(s.shape)}")
        if sn < 2 or su < n * sn:
            raise ValueError("samples_out: overlapping samples or units")
    l00, l10, l11 = _noise_factor(noise_cov, chol)
    mask = 2 ** 64 - 1
    args = (ctypes.c_void_p(nominal.data_ptr()), O, T, nominal.stride(0), nominal.stride(1),
            u0, count, n, l00, l10, l11,
            ctypes.c_uint64(int(seed) & mask), ctypes.c_uint64(int(stream_offset) & mask),
            ctypes.c_int32(1 if zero_first_step else 0),
            ctypes.c_void_p(ego.data_ptr()), ego.stride(0),
            params.robot_radius, params.obstacle_radius, params.alpha, params.delta, params.epsilon,
            ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(status.data_ptr() if status is not None else None),
            ctypes.c_void_p(samples_out.data_ptr() if samples_out is not None else None), su, sn,
            ctypes.c_void_p(_stream_handle(dev, stream)))
    launch = PreparedLaunch(_native.lib().drcvar_sampled_halfspaces_f64, args,
                            (nominal, ego, out, status, samples_out))
    return launch, out


def sampled_halfspaces(nominal: torch.Tensor, ego: torch.Tensor, n_samples: int,
                       params: RiskParams = RiskParams(), **kwargs) -> torch.Tensor:
    """Mean / CVaR / DR-CVaR halfspaces of every (obstacle, step) unit from the NOMINAL paths: one
    launch draws each unit's ``n_samples`` Gaussian samples in registers and reduces them to the
    unit's record; no ``[O, T, N, 2]`` buffer exists (arguments: :func:`prepare_sampled_halfspaces`).

    The draw is bit for bit ``sample_trajectories_device`` / ``sample_units_device`` for the same
    seed and stream offset, and the record agrees with ``safe_halfspaces`` on that draw to
    rounding (a summation order of its own).  Measured against sampler + ``safe_halfspaces`` on
    one stream (profiles/sampled/sampled_times.json): C3 (10 x 20 x 1000) 6.5 us
    against 17.3 us, C4 (64 x 30 x 5000) 58.3 us against 74.5 us; C5 (256 x 50 x 10000) is NOT
    faster, 0.774 ms against 0.720 ms — above 8192 samples a unit takes a whole CU's registers, so
    nothing overlaps its selection — and saves only the 2.05 GB buffer.  Nothing dispatches
    between the two forms, the caller chooses.
    """
    launch, out = prepare_sampled_halfspaces(nominal, ego, n_samples, params, **kwargs)
    if out.numel() > 0:
        launch()
    return out


def check_step_state(state, device: torch.device) -> None:
    """``state`` of the device-state entries: an int64 device tensor ``[stream_offset, step]``
    (``_native.StepState``; the offset as its two's-complement bit pattern), 16-byte aligned."""
    if not isinstance(state, torch.Tensor) or state.dtype != torch.int64:
        raise ValueError("state must be an int64 tensor [stream_offset, step]")
    if state.device != device:
        raise ValueError(f"state must live on {device}, got {state.device}")
    if tuple(state.shape) != (2,) or not state.is_contiguous():
        raise ValueError(f"state must be a contiguous tensor of 2 elements, got {tuple(state.shape)}")
    if state.data_ptr() % 16 != 0:
        raise ValueError("state must be 16-byte aligned")


def check_path(t, name: str, shape, device=None) -> None:
    """A whole path of the device-state entries, 2-D or (obstacles or problems first) 3-D: a
    float64 tensor of ``shape`` (None = any size) with a contiguous last dimension, on the GPU (``device``, when given).  Dtype and shape are
    checked before the device."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
        raise ValueError(f"{name} must be a float64 tensor")
    if t.dim() != len(shape) or any(w is not None and w != g for w, g in zip(shape, t.shape)):
        raise ValueError(f"{name} must have shape {list(shape)}, got {tuple(t.shape)}")
    if t.shape[0] < 1 or (t.dim() == 3 and t.shape[1] < 1):
        raise ValueError(f"{name}: a path needs at least one row")
    if t.stride(-1) != 1:
        raise ValueError(f"{name}: the last dimension must be contiguous")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must live on the GPU (HIP device tensor); the engine has no CPU path")
    if device is not None and t.device != device:
        raise ValueError(f"{name} must live on {device}, got {t.device}")


def prepare_sampled_halfspaces_dev(nominal_path: torch.Tensor, ego_path: torch.Tensor, n_steps: int,
                                   n_samples: int, params: RiskParams, state: torch.Tensor,
                                   noise_cov=DEFAULT_NOISE_COV, seed: int = 0,
                                   zero_first_step: bool = True, unit_begin: int = 0,
                                   unit_count: int | None = None, out: torch.Tensor | None = None,
                                   status: torch.Tensor | None = None, stream=None,
                                   chol=None) -> tuple[PreparedLaunch, torch.Tensor]:
    """Freeze one ``drcvar_sampled_halfspaces_f64_dev`` call: :func:`prepare_sampled_halfspaces` on
    the window of ``n_steps`` rows that starts at ``state[1]``, drawn with the stream offset
    ``state[0]`` — both read from device memory when the kernel runs, so a graph that captured
    the launch follows ``state`` from replay to replay.

    nominal_path ``[O, P, 2]`` and ego_path ``[P, 2]`` float64 device tensors with adjacent
    coordinates (whole paths, ``P >= 1``); window row ``t`` is path row ``min(max(step + t, 0),
    P - 1)``.  ``state``: :func:`check_step_state`.  The records and status words are bit for bit
    those of :func:`sampled_halfspaces` on the gathered window with that offset; the other arguments
    are its own (``out`` is ``[O, n_steps, 8]``, or ``[unit_count, 8]`` for a unit window)."""
    params.validate()
    if not isinstance(nominal_path, torch.Tensor) or nominal_path.dim() != 3 or nominal_path.shape[0] < 1:
        raise ValueError("nominal_path must be float64 [O, P, 2] with O, P >= 1")
    check_path(nominal_path, "nominal_path", (None, None, 2))
    dev = nominal_path.device
    O, P, _ = nominal_path.shape
    check_path(ego_path, "ego_path", (P, 2), dev)
    check_step_state(state, dev)
    T, n = int(n_steps), int(n_samples)
    if T < 0:
        raise ValueError(f"n_steps={T} must not be negative")
    if n < 1 or n > _native.MAX_SAMPLES:
        raise ValueError(f"n_samples={n} outside 1..{_native.MAX_SAMPLES}")
    whole = unit_count is None
    u0 = int(unit_begin)
    count = O * T - u0 if whole else int(unit_count)
    if u0 < 0 or count < 0 or u0 + count > O * T:
        raise ValueError(f"unit range [{u0}, {u0 + count}) outside the {O} x {T} grid")
    whole = whole and u0 == 0
    shape = (O, T, OUT_WIDTH) if whole else (count, OUT_WIDTH)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=dev)
    else:
        _check_out(out, shape, dev, "[O, T, 8]" if whole else "[units, 8]")
    if status is not None:
        _check_status(status, count, dev)
    l00, l10, l11 = _noise_factor(noise_cov, chol)
    args = (ctypes.c_void_p(nominal_path.data_ptr()), O, P, nominal_path.stride(0),
            nominal_path.stride(1), T, u0, count, n, l00, l10, l11,
            ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), ctypes.c_void_p(state.data_ptr()),
            ctypes.c_int32(1 if zero_first_step else 0),
            ctypes.c_void_p(ego_path.data_ptr()), ego_path.stride(0),
            params.robot_radius, params.obstacle_radius, params.alpha, params.delta, params.epsilon,
            ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(status.data_ptr() if status is not None else None),
            ctypes.c_void_p(_stream_handle(dev, stream)))
    launch = PreparedLaunch(_native.lib().drcvar_sampled_halfspaces_f64_dev, args,
                            (nominal_path, ego_path, state, out, status))
    return launch, out


def sampled_halfspaces_dev(nominal_path: torch.Tensor, ego_path: torch.Tensor, n_steps: int,
                           n_samples: int, params: RiskParams, state: torch.Tensor,
                           **kwargs) -> torch.Tensor:
    """One ``drcvar_sampled_halfspaces_f64_dev`` launch (arguments:
    :func:`prepare_sampled_halfspaces_dev`): the halfspaces of the window that ``state`` names."""
    launch, out = prepare_sampled_halfspaces_dev(nominal_path, ego_path, n_steps, n_samples, params,
                                                 state, **kwargs)
    if out.numel() > 0:
        launch()
    return out


def prepare_sampled_halfspaces_pred(nominal_path: torch.Tensor, x0: torch.Tensor, pred: torch.Tensor,
                                    c_out, n_obstacles: int, n_steps: int, n_samples: int,
                                    params: RiskParams, state: torch.Tensor, *, shift: int = 1,
                                    noise_cov=DEFAULT_NOISE_COV, seed: int = 0,
                                    zero_first_step: bool = True, unit_begin: int = 0,
                                    unit_count: int | None = None, out: torch.Tensor | None = None,
                                    status: torch.Tensor | None = None, stream=None,
                                    chol=None) -> tuple[PreparedLaunch, torch.Tensor]:
    """Freeze one ``drcvar_sampled_halfspaces_f64_pred`` call (``include/drcvar_loop_pred.h``):
    :func:`prepare_sampled_halfspaces_dev` for B problems of ``n_obstacles`` = O obstacles each,
    with the ego of every unit taken from its own problem's state and predicted path instead of
    one shared ego path.

    nominal_path ``[B O, P, 2]`` (problem b's obstacles are rows ``b O .. b O + O - 1``), x0 ``[B,
    nx]`` and pred ``[B, R, nx]`` (``R >= 1``, ``1 <= nx <= 8``) are float64 device tensors, x0 and
    pred contiguous; ``c_out`` is a host ``[2, nx]`` array, copied when this function is called.
    Unit ``u = (b O + o) T + t`` draws what :func:`sampled_halfspaces_dev` draws and takes the ego
    ``c_out @ xs`` (an fma chain from +0.0), ``xs = x0[b]`` at ``t = 0`` and ``pred[b, min(t +
    shift, R - 1)]`` after it, ``shift`` 0 or 1: x0, pred and ``state`` are read from device memory
    when the kernel runs, so a captured launch follows them.  Per problem the records and status
    words are bit for bit those of :func:`sampled_halfspaces` on the gathered window with that ego,
    ``unit_begin = b O T``, ``unit_count = O T`` and the state's offset.  ``out`` is ``[B O,
    n_steps, 8]``, or ``[unit_count, 8]`` for a unit window; ``status``, ``stream`` and ``chol`` as
    in :func:`prepare_sampled_halfspaces_dev`."""
    params.validate()
    if not isinstance(nominal_path, torch.Tensor) or nominal_path.dim() != 3 or nominal_path.shape[0] < 1:
        raise ValueError("nominal_path must be float64 [B O, P, 2] with B O, P >= 1")
    check_path(nominal_path, "nominal_path", (None, None, 2))
    dev = nominal_path.device
    BO, P, _ = nominal_path.shape
    O = int(n_obstacles)
    if O < 1 or BO % O != 0:
        raise ValueError(f"n_obstacles={O} must be at least 1 and divide nominal_path's {BO} rows")
    B = BO // O
    if not isinstance(x0, torch.Tensor) or x0.dim() != 2:
        raise ValueError("x0 must be a float64 [B, nx] tensor")
    nx = x0.shape[1]
    if not 1 <= nx <= _native.MPC_MAX_STATES:
        raise ValueError(f"x0 has {nx} states, outside 1..{_native.MPC_MAX_STATES}")
    check_path(x0, "x0", (B, nx), dev)
    if not isinstance(pred, torch.Tensor) or pred.dim() != 3:
        raise ValueError("pred must be a float64 [B, R, nx] tensor")
    check_path(pred, "pred", (B, None, nx), dev)
    if not x0.is_contiguous() or not pred.is_contiguous():
        raise ValueError("x0 and pred must be contiguous")
    import numpy as np
    c = np.ascontiguousarray(np.asarray(c_out, dtype=np.float64))
    if c.shape != (2, nx):
        raise ValueError(f"c_out must have shape (2, {nx}), got {c.shape}")
    if int(shift) not in (0, 1):
        raise ValueError(f"shift={shift} must be 0 or 1")
    check_step_state(state, dev)
    T, n = int(n_steps), int(n_samples)
    if T < 0:
        raise ValueError(f"n_steps={T} must not be negative")
    if n < 1 or n > _native.MAX_SAMPLES:
        raise ValueError(f"n_samples={n} outside 1..{_native.MAX_SAMPLES}")
    whole = unit_count is None
    u0 = int(unit_begin)
    count = BO * T - u0 if whole else int(unit_count)
    if u0 < 0 or count < 0 or u0 + count > BO * T:
        raise ValueError(f"unit range [{u0}, {u0 + count}) outside the {BO} x {T} grid")
    whole = whole and u0 == 0
    shape = (BO, T, OUT_WIDTH) if whole else (count, OUT_WIDTH)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=dev)
    else:
        _check_out(out, shape, dev, "[B O, T, 8]" if whole else "[units, 8]")
    if status is not None:
        _check_status(status, count, dev)
    l00, l10, l11 = _noise_factor(noise_cov, chol)
    args = (ctypes.c_void_p(nominal_path.data_ptr()), BO, P, nominal_path.stride(0),
            nominal_path.stride(1), T, u0, count, n, l00, l10, l11,
            ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), ctypes.c_void_p(state.data_ptr()),
            ctypes.c_int32(1 if zero_first_step else 0), O,
            ctypes.c_void_p(x0.data_ptr()), ctypes.c_void_p(pred.data_ptr()), pred.shape[1],
            ctypes.c_int32(nx), ctypes.c_void_p(c.ctypes.data), ctypes.c_int32(int(shift)),
            params.robot_radius, params.obstacle_radius, params.alpha, params.delta, params.epsilon,
            ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(status.data_ptr() if status is not None else None),
            ctypes.c_void_p(_stream_handle(dev, stream)))
    launch = PreparedLaunch(_native.pred_lib().drcvar_sampled_halfspaces_f64_pred, args,
                            (nominal_path, x0, pred, c, state, out, status))
    return launch, out


def sampled_halfspaces_pred(nominal_path: torch.Tensor, x0: torch.Tensor, pred: torch.Tensor, c_out,
                            n_obstacles: int, n_steps: int, n_samples: int, params: RiskParams,
                            state: torch.Tensor, **kwargs) -> torch.Tensor:
    """One ``drcvar_sampled_halfspaces_f64_pred`` launch (arguments:
    :func:`prepare_sampled_halfspaces_pred`): the halfspaces of the window that ``state`` names,
    each problem's about its own state and predicted path."""
    launch, out = prepare_sampled_halfspaces_pred(nominal_path, x0, pred, c_out, n_obstacles,
                                                  n_steps, n_samples, params, state, **kwargs)
    if out.numel() > 0:
        launch()
    return out


@dataclass(frozen=True)
class RiskTable:
    """Risk parameters per problem of a batch (``include/drcvar_loop_risk.h``): ``alpha``,
    ``delta`` and ``epsilon`` are each a scalar or a sequence of one length B, broadcast to B
    (B = 1 when all three are scalars); the radii are scalars."""

    alpha: object = 0.2
    delta: object = 0.1
    epsilon: object = 0.15
    robot_radius: float = 0.3
    obstacle_radius: float = 0.3

    def _columns(self):
        """(alpha, delta, epsilon) as float64 arrays ``[B]``."""
        import numpy as np
        cols = [np.asarray(v, dtype=np.float64) for v in (self.alpha, self.delta, self.epsilon)]
        if any(c.ndim > 1 for c in cols):
            raise ValueError("alpha, delta and epsilon must be scalars or one-dimensional")
        lengths = {c.shape[0] for c in cols if c.ndim == 1}
        if len(lengths) > 1:
            raise ValueError(f"alpha, delta and epsilon have different lengths {sorted(lengths)}")
        B = lengths.pop() if lengths else 1
        return tuple(np.ascontiguousarray(np.broadcast_to(c, (B,))) for c in cols)

    def __len__(self) -> int:
        return int(self._columns()[0].shape[0])

    def validate(self) -> None:
        alpha, delta, epsilon = self._columns()
        if alpha.shape[0] < 1:
            raise ValueError("a risk table needs at least one row")
        radii = (float(self.robot_radius), float(self.obstacle_radius))
        if not all(math.isfinite(v) for v in (*radii, *alpha, *delta, *epsilon)):
            raise ValueError(f"risk parameters must be finite: {self}")
        if not (alpha > 0.0).all():
            raise ValueError(f"alpha must be > 0 in every row, got {alpha.tolist()}")

    def row(self, b: int) -> RiskParams:
        """Problem ``b``'s parameters as the launch-uniform entries take them."""
        alpha, delta, epsilon = self._columns()
        return RiskParams(float(self.robot_radius), float(self.obstacle_radius), float(alpha[b]),
                          float(delta[b]), float(epsilon[b]))

    def to_device(self, n_samples: int, device) -> torch.Tensor:
        """The filled table for ``n_samples`` as a uint8 tensor ``[B, row_bytes]`` on ``device``
        (``drcvar_risk_table_fill`` into host memory, one copy): a table belongs to one
        ``n_samples``."""
        import numpy as np
        self.validate()
        alpha, delta, epsilon = self._columns()
        B = alpha.shape[0]
        lib = _native.risk_lib()
        row = int(lib.drcvar_risk_table_row_bytes())
        host = np.zeros((B, row), dtype=np.uint8)
        _native.check(lib.drcvar_risk_table_fill(
            alpha.ctypes.data, delta.ctypes.data, epsilon.ctypes.data, B, float(self.robot_radius),
            float(self.obstacle_radius), int(n_samples), host.ctypes.data, host.nbytes))
        return torch.from_numpy(host).to(device)


def _risk_launch_setup(nominal_path, ego_path, n_obstacles, n_steps, n_samples, params, state,
                       draw_period, table, noise_cov, unit_begin, unit_count, out, status, chol,
                       routes=False):
    """The checks and launch-uniform values that the risk-table, the metric and the route launch
    share (:func:`prepare_sampled_halfspaces_risk`): ``(dev, BO, P, O, B, D, T, n, u0, count, whole,
    out, table, (l00, l10, l11))``.  ``routes``: ego_path is ``[B, P, 2]``, a path per problem."""
    if not isinstance(params, RiskTable):
        raise ValueError("params must be a RiskTable")
    params.validate()
    if not isinstance(nominal_path, torch.Tensor) or nominal_path.dim() != 3 or nominal_path.shape[0] < 1:
        raise ValueError("nominal_path must be float64 [B O, P, 2] with B O, P >= 1")
    check_path(nominal_path, "nominal_path", (None, None, 2))
    dev = nominal_path.device
    BO, P, _ = nominal_path.shape
    O = int(n_obstacles)
    if O < 1 or BO % O != 0:
        raise ValueError(f"n_obstacles={O} must be at least 1 and divide nominal_path's {BO} rows")
    B = BO // O
    if len(params) != B:
        raise ValueError(f"the risk table has {len(params)} rows, the launch {B} problems")
    D = B if draw_period is None else int(draw_period)
    if D < 1:
        raise ValueError(f"draw_period={draw_period} must be at least 1")
    check_path(ego_path, "ego_path", (B, P, 2) if routes else (P, 2), dev)
    check_step_state(state, dev)
    T, n = int(n_steps), int(n_samples)
    if T < 0:
        raise ValueError(f"n_steps={T} must not be negative")
    if n < 1 or n > _native.MAX_SAMPLES:
        raise ValueError(f"n_samples={n} outside 1..{_native.MAX_SAMPLES}")
    whole = unit_count is None
    u0 = int(unit_begin)
    count = BO * T - u0 if whole else int(unit_count)
    if u0 < 0 or count < 0 or u0 + count > BO * T:
        raise ValueError(f"unit range [{u0}, {u0 + count}) outside the {BO} x {T} grid")
    whole = whole and u0 == 0
    shape = (BO, T, OUT_WIDTH) if whole else (count, OUT_WIDTH)
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=dev)
    else:
        _check_out(out, shape, dev, "[B O, T, 8]" if whole else "[units, 8]")
    if status is not None:
        _check_status(status, count, dev)
    if table is None:
        table = params.to_device(n, dev)
    row = int(_native.risk_lib().drcvar_risk_table_row_bytes())
    if not isinstance(table, torch.Tensor) or table.dtype != torch.uint8 or table.device != dev or \
            tuple(table.shape) != (B, row) or not table.is_contiguous() or table.data_ptr() % 16 != 0:
        raise ValueError(f"table must be a contiguous, 16-byte aligned uint8 [{B}, {row}] tensor on "
                         f"{dev} (RiskTable.to_device)")
    l00, l10, l11 = _noise_factor(noise_cov, chol)
    return dev, BO, P, O, B, D, T, n, u0, count, whole, out, table, (l00, l10, l11)


def prepare_sampled_halfspaces_risk(nominal_path: torch.Tensor, ego_path: torch.Tensor,
                                    n_obstacles: int, n_steps: int, n_samples: int,
                                    params: RiskTable, state: torch.Tensor, *,
                                    draw_period: int | None = None, table: torch.Tensor | None = None,
                                    noise_cov=DEFAULT_NOISE_COV, seed: int = 0,
                                    zero_first_step: bool = True, unit_begin: int = 0,
                                    unit_count: int | None = None, out: torch.Tensor | None = None,
                                    status: torch.Tensor | None = None, stream=None,
                                    chol=None) -> tuple[PreparedLaunch, torch.Tensor]:
    """Freeze one ``drcvar_sampled_halfspaces_f64_risk`` call (``include/drcvar_loop_risk.h``):
    :func:`prepare_sampled_halfspaces_dev` for B problems of ``n_obstacles`` = O obstacles each,
    with the risk parameters of every unit taken from its own problem's row of ``params`` (a
    :class:`RiskTable` of B rows) and draws shared between problems by ``draw_period``.

    nominal_path ``[B O, P, 2]`` (problem b's obstacles are rows ``b O .. b O + O - 1``) and
    ego_path ``[P, 2]`` as in :func:`prepare_sampled_halfspaces_dev`.  Unit ``u = (b O + o) T + t``
    takes what that entry's unit takes, but filters with ``params.row(b)`` and draws the Philox
    counters of unit ``((b mod D) O + o) T + t``, ``D = draw_period`` (None: B, the entry's own
    draws; 1: every problem meets problem 0's draws; B = S D with ``b = s D + r``: S settings on
    the same D replicate draws).  Per problem the records and status words are bit for bit those of
    :func:`sampled_halfspaces` on a nominal tensor whose rows ``(b mod D) O .. + O`` are the
    problem's gathered window, with the gathered ego window, ``unit_begin = (b mod D) O T``,
    ``unit_count = O T``, the state's offset and ``params.row(b)``.

    ``table`` (optional): ``params.to_device(n_samples, device)`` made earlier, so that several
    launches share one copy; the entry cannot check device memory, so the table is only accepted
    with the shape that ``params`` and the library give it.  ``out`` is ``[B O, n_steps, 8]``, or
    ``[unit_count, 8]`` for a unit window; ``status``, ``stream`` and ``chol`` as in
    :func:`prepare_sampled_halfspaces_dev`."""
    dev, BO, P, O, B, D, T, n, u0, count, whole, out, table, (l00, l10, l11) = _risk_launch_setup(
        nominal_path, ego_path, n_obstacles, n_steps, n_samples, params, state, draw_period, table,
        noise_cov, unit_begin, unit_count, out, status, chol)
    args = (ctypes.c_void_p(nominal_path.data_ptr()), BO, P, nominal_path.stride(0),
            nominal_path.stride(1), T, u0, count, n, l00, l10, l11,
            ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), ctypes.c_void_p(state.data_ptr()),
            ctypes.c_int32(1 if zero_first_step else 0),
            ctypes.c_void_p(ego_path.data_ptr()), ego_path.stride(0), O,
            ctypes.c_void_p(table.data_ptr()), D, ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(status.data_ptr() if status is not None else None),
            ctypes.c_void_p(_stream_handle(dev, stream)))
    launch = PreparedLaunch(_native.risk_lib().drcvar_sampled_halfspaces_f64_risk, args,
                            (nominal_path, ego_path, state, table, out, status))
    return launch, out


def sampled_halfspaces_risk(nominal_path: torch.Tensor, ego_path: torch.Tensor, n_obstacles: int,
                            n_steps: int, n_samples: int, params: RiskTable, state: torch.Tensor,
                            **kwargs) -> torch.Tensor:
    """One ``drcvar_sampled_halfspaces_f64_risk`` launch (arguments:
    :func:`prepare_sampled_halfspaces_risk`): the halfspaces of the window that ``state`` names,
    each problem's with its own risk parameters."""
    launch, out = prepare_sampled_halfspaces_risk(nominal_path, ego_path, n_obstacles, n_steps,
                                                  n_samples, params, state, **kwargs)
    if out.numel() > 0:
        launch()
    return out


METRIC_CODES = {"mean": 0, "cvar": 1, "dr_cvar": 2}   # DRCVAR_METRIC_* (include/drcvar_loop_metric.h)
SELECTED_WIDTH = 4                                    # DRCVAR_SEL_WIDTH


def metric_codes(metric, n_problems: int, device) -> torch.Tensor:
    """The names ``metric`` (a sequence of ``n_problems`` keys of :data:`METRIC_CODES`) as the
    int32 ``[B]`` tensor on ``device`` that the metric launch reads."""
    if isinstance(metric, str) or not hasattr(metric, "__len__"):
        raise ValueError("metric must be a sequence of names, one per problem")
    names = list(metric)
    if len(names) != int(n_problems):
        raise ValueError(f"metric has {len(names)} names, the launch {n_problems} problems")
    unknown = [m for m in names if not isinstance(m, str) or m not in METRIC_CODES]
    if unknown:
        raise ValueError(f"metric names must be among {tuple(METRIC_CODES)}, got {unknown[0]!r}")
    return torch.tensor([METRIC_CODES[m] for m in names], dtype=torch.int32).to(device)


def prepare_sampled_halfspaces_metric(nominal_path: torch.Tensor, ego_path: torch.Tensor,
                                      n_obstacles: int, n_steps: int, n_samples: int,
                                      params: RiskTable, metric, state: torch.Tensor, *,
                                      draw_period: int | None = None,
                                      table: torch.Tensor | None = None,
                                      codes: torch.Tensor | None = None,
                                      noise_cov=DEFAULT_NOISE_COV, seed: int = 0,
                                      zero_first_step: bool = True, unit_begin: int = 0,
                                      unit_count: int | None = None, out: torch.Tensor | None = None,
                                      selected: torch.Tensor | None = None,
                                      status: torch.Tensor | None = None, stream=None, chol=None,
                                      _routes: bool = False
                                      ) -> tuple[PreparedLaunch, torch.Tensor, torch.Tensor]:
    """Freeze one ``drcvar_sampled_halfspaces_f64_metric`` call (``include/drcvar_loop_metric.h``):
    :func:`prepare_sampled_halfspaces_risk` whose launch also writes, for every unit, the halfspace
    under its own problem's metric.  Returns ``(launch, out, selected)``.

    ``metric`` is a sequence of B names among :data:`METRIC_CODES`.  ``out`` and ``status`` are
    byte for byte what :func:`prepare_sampled_halfspaces_risk` gives for the same arguments;
    ``selected`` is ``[B O, n_steps, 4]`` (``[unit_count, 4]`` for a unit window): for a unit of
    problem b the columns ``core/mpc_filter.METRIC_COLUMNS[metric[b]]`` of its record, then +0.0,
    stored by the lane that stores the record (:func:`selected_views` gives the solver's views).

    ``codes`` (optional): ``metric_codes(metric, B, device)`` made earlier, as ``table`` is for the
    rows; the entry cannot check device memory, so it is only accepted as an int32 ``[B]`` tensor
    on the device.  Everything else: :func:`prepare_sampled_halfspaces_risk`."""
    if isinstance(nominal_path, torch.Tensor) and nominal_path.dim() == 3 and int(n_obstacles) >= 1 \
            and nominal_path.shape[0] % int(n_obstacles) == 0:
        # what the host alone can tell about metric, codes and selected, before anything else: the
        # names, and the shapes the kernel would read and write through the raw pointers
        rows, B = nominal_path.shape[0], nominal_path.shape[0] // int(n_obstacles)
        metric_codes(metric, B, "cpu")
        if codes is not None and (not isinstance(codes, torch.Tensor) or codes.dtype != torch.int32
                                  or tuple(codes.shape) != (B,) or not codes.is_contiguous()):
            raise ValueError(f"codes must be a contiguous int32 [{B}] tensor (metric_codes)")
        if selected is not None:
            if unit_count is None and int(unit_begin) == 0:
                shape = (rows, int(n_steps), SELECTED_WIDTH)
            else:
                shape = (rows * int(n_steps) - int(unit_begin) if unit_count is None else int(unit_count),
                         SELECTED_WIDTH)
            if not isinstance(selected, torch.Tensor) or tuple(selected.shape) != shape or \
                    selected.dtype != torch.float64 or not selected.is_contiguous():
                raise ValueError(f"selected must be a contiguous float64 {list(shape)} tensor")
    dev, BO, P, O, B, D, T, n, u0, count, whole, out, table, (l00, l10, l11) = _risk_launch_setup(
        nominal_path, ego_path, n_obstacles, n_steps, n_samples, params, state, draw_period, table,
        noise_cov, unit_begin, unit_count, out, status, chol, routes=_routes)
    if codes is None:
        codes = metric_codes(metric, B, dev)
    elif codes.device != dev:
        raise ValueError(f"codes must live on {dev}")
    if selected is None:
        selected = torch.empty((BO, T, SELECTED_WIDTH) if whole else (count, SELECTED_WIDTH),
                               dtype=torch.float64, device=dev)
    elif selected.device != dev:
        raise ValueError(f"selected must live on {dev}")
    # (the route launch: the same arguments, and the ego path's two strides in place of one)
    ego_strides = (ego_path.stride(1), ego_path.stride(0)) if _routes else (ego_path.stride(0),)
    entry = _native.route_lib().drcvar_sampled_halfspaces_f64_route if _routes else \
        _native.metric_lib().drcvar_sampled_halfspaces_f64_metric
    args = (ctypes.c_void_p(nominal_path.data_ptr()), BO, P, nominal_path.stride(0),
            nominal_path.stride(1), T, u0, count, n, l00, l10, l11,
            ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), ctypes.c_void_p(state.data_ptr()),
            ctypes.c_int32(1 if zero_first_step else 0),
            ctypes.c_void_p(ego_path.data_ptr()), *ego_strides, O,
            ctypes.c_void_p(table.data_ptr()), D, ctypes.c_void_p(codes.data_ptr()),
            ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(status.data_ptr() if status is not None else None),
            ctypes.c_void_p(selected.data_ptr()), ctypes.c_void_p(_stream_handle(dev, stream)))
    launch = PreparedLaunch(entry, args,
                            (nominal_path, ego_path, state, table, codes, out, status, selected))
    return launch, out, selected


def sampled_halfspaces_metric(nominal_path: torch.Tensor, ego_path: torch.Tensor, n_obstacles: int,
                              n_steps: int, n_samples: int, params: RiskTable, metric,
                              state: torch.Tensor, **kwargs) -> tuple[torch.Tensor, torch.Tensor]:
    """One ``drcvar_sampled_halfspaces_f64_metric`` launch (arguments:
    :func:`prepare_sampled_halfspaces_metric`): returns ``(out, selected)``."""
    launch, out, selected = prepare_sampled_halfspaces_metric(
        nominal_path, ego_path, n_obstacles, n_steps, n_samples, params, metric, state, **kwargs)
    if out.numel() > 0:
        launch()
    return out, selected


def prepare_sampled_halfspaces_route(nominal_path: torch.Tensor, ego_path: torch.Tensor,
                                     n_obstacles: int, n_steps: int, n_samples: int,
                                     params: RiskTable, metric, state: torch.Tensor, **kwargs
                                     ) -> tuple[PreparedLaunch, torch.Tensor, torch.Tensor]:
    """Freeze one ``drcvar_sampled_halfspaces_f64_route`` call (``include/drcvar_loop_route.h``):
    :func:`prepare_sampled_halfspaces_metric` with an ego path per problem.  Returns ``(launch,
    out, selected)``.

    ``ego_path`` is ``[B, P, 2]`` with adjacent coordinates and any problem and row strides (an
    expanded path, problem stride 0, is the metric launch's one path); the ego of unit ``(b O + o)
    T + t`` is ``ego_path[b, c(step + t)]``.  Per problem b, ``out``, ``status`` and ``selected``
    hold byte for byte what :func:`prepare_sampled_halfspaces_metric` gives for the unit window
    ``[b O T, (b + 1) O T)`` with ``ego_path[b]``.  Negative strides are a ``ValueError``.
    Everything else, keyword arguments included: :func:`prepare_sampled_halfspaces_metric`."""
    # what the host alone can tell about ego_path, before anything else: the shape the kernel
    # would read through the raw pointer and the two strides
    if not isinstance(ego_path, torch.Tensor) or ego_path.dtype != torch.float64 or \
            ego_path.dim() != 3 or ego_path.shape[2] != 2 or ego_path.stride(2) != 1:
        raise ValueError("ego_path must be a float64 [B, P, 2] tensor with adjacent coordinates")
    if isinstance(nominal_path, torch.Tensor) and nominal_path.dim() == 3 and int(n_obstacles) >= 1 \
            and nominal_path.shape[0] % int(n_obstacles) == 0:
        want = (nominal_path.shape[0] // int(n_obstacles), nominal_path.shape[1], 2)
        if tuple(ego_path.shape) != want:
            raise ValueError(f"ego_path must have shape {list(want)}, got {tuple(ego_path.shape)}")
    if ego_path.stride(0) < 0 or ego_path.stride(1) < 0:
        raise ValueError("ego_path must not have negative strides")
    return prepare_sampled_halfspaces_metric(nominal_path, ego_path, n_obstacles, n_steps, n_samples,
                                             params, metric, state, _routes=True, **kwargs)


def sampled_halfspaces_route(nominal_path: torch.Tensor, ego_path: torch.Tensor, n_obstacles: int,
                             n_steps: int, n_samples: int, params: RiskTable, metric,
                             state: torch.Tensor, **kwargs) -> tuple[torch.Tensor, torch.Tensor]:
    """One ``drcvar_sampled_halfspaces_f64_route`` launch (arguments:
    :func:`prepare_sampled_halfspaces_route`): returns ``(out, selected)``."""
    launch, out, selected = prepare_sampled_halfspaces_route(
        nominal_path, ego_path, n_obstacles, n_steps, n_samples, params, metric, state, **kwargs)
    if out.numel() > 0:
        launch()
    return out, selected


@dataclass(frozen=True)
class NoiseTable:
    """Noise factors per look-ahead step of a batch (``include/drcvar_loop_noise.h``): ``chol`` is
    an array of lower Cholesky factors ``(l00, l10, l11)`` shaped ``[H, 3]`` (one schedule for every
    obstacle), ``[O, H, 3]`` (one per obstacle, shared by the problems) or ``[B, O, H, 3]`` (one
    per problem and obstacle).  A factor may be zero, singular or infinite, never NaN."""

    chol: object

    def _array(self):
        import numpy as np
        c = np.ascontiguousarray(np.asarray(self.chol, dtype=np.float64))
        if c.ndim not in (2, 3, 4) or c.shape[-1] != 3 or any(d < 1 for d in c.shape):
            raise ValueError("chol must have shape [H, 3], [O, H, 3] or [B, O, H, 3] with H >= 1, "
                             f"got {tuple(c.shape)}")
        return c

    @classmethod
    def from_cov(cls, cov) -> "NoiseTable":
        """The table of the covariances ``cov [..., H, 2, 2]``: each factor formed as
        ``np.linalg.cholesky`` forms it (what the entries with ``noise_cov`` do)."""
        import numpy as np
        cov = np.asarray(cov, dtype=np.float64)
        if cov.ndim not in (3, 4, 5) or cov.shape[-2:] != (2, 2):
            raise ValueError(f"cov must have shape [..., H, 2, 2], got {tuple(cov.shape)}")
        flat = cov.reshape(-1, 2, 2)
        chol = np.array([_noise_factor(c, None) for c in flat]).reshape(*cov.shape[:-2], 3)
        return cls(chol)

    @classmethod
    def scaled(cls, noise_cov, scales) -> "NoiseTable":
        """``Sigma = scale * noise_cov`` for ``scales [..., H]``; a scale of 1 gives the factor of
        ``noise_cov`` itself, bit for bit."""
        import numpy as np
        scales = np.asarray(scales, dtype=np.float64)
        base = np.asarray(noise_cov, dtype=np.float64).reshape(2, 2)
        return cls.from_cov(scales[..., None, None] * base)

    @property
    def horizon(self) -> int:
        return int(self._array().shape[-2])

    def validate(self) -> None:
        import numpy as np
        if np.isnan(self._array()).any():
            raise ValueError("a noise factor must not be NaN")

    def period(self, n_problems: int, n_obstacles: int) -> int:
        """The launch's ``noise_period`` for B problems of O obstacles: 1, O or B O by the table's
        leading dimensions, which must match."""
        B, O = int(n_problems), int(n_obstacles)
        lead = self._array().shape[:-2]
        if lead == ():
            return 1
        if lead == (O,):
            return O
        if lead == (B, O):
            return B * O
        raise ValueError(f"the noise table's leading dimensions {lead} match neither "
                         f"n_obstacles={O} nor (n_problems, n_obstacles)={(B, O)}")

    def factor(self, o: int, t: int):
        """``(l00, l10, l11)`` of global obstacle ``o`` at window step ``t``."""
        c = self._array()
        rows = c.reshape(-1, c.shape[-2], 3)
        return tuple(float(v) for v in rows[int(o) % rows.shape[0], int(t)])

    def to_device(self, device) -> torch.Tensor:
        """The filled table as a uint8 tensor ``[period * H, row_bytes]`` on ``device``
        (``drcvar_noise_table_fill`` into host memory, one copy)."""
        import numpy as np
        self.validate()
        c = self._array().reshape(-1, 3)
        lib = _native.noise_lib()
        row = int(lib.drcvar_noise_table_row_bytes())
        host = np.zeros((c.shape[0], row), dtype=np.uint8)
        _native.check(lib.drcvar_noise_table_fill(c.ctypes.data, c.shape[0], host.ctypes.data,
                                                  host.nbytes))
        return torch.from_numpy(host).to(device)


def prepare_sampled_halfspaces_noise(nominal_path: torch.Tensor, ego_path: torch.Tensor,
                                     n_obstacles: int, n_steps: int, n_samples: int,
                                     params: RiskTable, metric, state: torch.Tensor,
                                     noise: NoiseTable, *, noise_table: torch.Tensor | None = None,
                                     draw_period: int | None = None,
                                     table: torch.Tensor | None = None,
                                     codes: torch.Tensor | None = None, seed: int = 0,
                                     zero_first_step: bool = True, unit_begin: int = 0,
                                     unit_count: int | None = None, out: torch.Tensor | None = None,
                                     selected: torch.Tensor | None = None,
                                     status: torch.Tensor | None = None, stream=None
                                     ) -> tuple[PreparedLaunch, torch.Tensor, torch.Tensor]:
    """Freeze one ``drcvar_sampled_halfspaces_f64_noise`` call (``include/drcvar_loop_noise.h``):
    :func:`prepare_sampled_halfspaces_route` whose unit ``(o, t)`` draws with its own factor
    ``noise.factor(o, t)`` instead of one ``noise_cov`` / ``chol`` per launch.  Returns ``(launch,
    out, selected)``.

    ``noise`` is a :class:`NoiseTable` whose H is ``n_steps`` and whose leading dimensions match
    ``n_obstacles`` or ``(B, n_obstacles)``.  For every unit, ``out``, ``status`` and ``selected``
    hold byte for byte what :func:`prepare_sampled_halfspaces_route` gives with ``chol`` that
    unit's factor.  ``noise_table`` (optional): ``noise.to_device(device)`` made earlier; the entry
    cannot check device memory, so it is only accepted with the shape that ``noise`` and the
    library give it.  Everything else: :func:`prepare_sampled_halfspaces_route` (there is no
    ``noise_cov`` and no ``chol``)."""
    if not isinstance(noise, NoiseTable):
        raise ValueError("noise must be a NoiseTable")
    noise.validate()
    if noise.horizon != int(n_steps):
        raise ValueError(f"the noise table has H={noise.horizon}, the launch n_steps={n_steps}")
    if not isinstance(ego_path, torch.Tensor) or ego_path.dtype != torch.float64 or \
            ego_path.dim() != 3 or ego_path.shape[2] != 2 or ego_path.stride(2) != 1:
        raise ValueError("ego_path must be a float64 [B, P, 2] tensor with adjacent coordinates")
    if ego_path.stride(0) < 0 or ego_path.stride(1) < 0:
        raise ValueError("ego_path must not have negative strides")
    if not isinstance(nominal_path, torch.Tensor) or nominal_path.dim() != 3 or \
            int(n_obstacles) < 1 or nominal_path.shape[0] % int(n_obstacles) != 0:
        raise ValueError("nominal_path must be float64 [B O, P, 2] with n_obstacles dividing B O")
    rows, T = nominal_path.shape[0], int(n_steps)
    period = noise.period(rows // int(n_obstacles), int(n_obstacles))
    metric_codes(metric, rows // int(n_obstacles), "cpu")
    if codes is not None and (not isinstance(codes, torch.Tensor) or codes.dtype != torch.int32
                              or tuple(codes.shape) != (rows // int(n_obstacles),)
                              or not codes.is_contiguous()):
        raise ValueError("codes must be a contiguous int32 [B] tensor (metric_codes)")
    dev, BO, P, O, B, D, T, n, u0, count, whole, out, table, _ = _risk_launch_setup(
        nominal_path, ego_path, n_obstacles, n_steps, n_samples, params, state, draw_period, table,
        DEFAULT_NOISE_COV, unit_begin, unit_count, out, status, None, routes=True)
    sel_shape = (BO, T, SELECTED_WIDTH) if whole else (count, SELECTED_WIDTH)
    if selected is None:
        selected = torch.empty(sel_shape, dtype=torch.float64, device=dev)
    elif not isinstance(selected, torch.Tensor) or tuple(selected.shape) != sel_shape or \
            selected.dtype != torch.float64 or not selected.is_contiguous() or selected.device != dev:
        raise ValueError(f"selected must be a contiguous float64 {list(sel_shape)} tensor on {dev}")
    if codes is None:
        codes = metric_codes(metric, B, dev)
    elif codes.device != dev:
        raise ValueError(f"codes must live on {dev}")
    lib = _native.noise_lib()
    if noise_table is None:
        noise_table = noise.to_device(dev)
    row = int(lib.drcvar_noise_table_row_bytes())
    if not isinstance(noise_table, torch.Tensor) or noise_table.dtype != torch.uint8 or \
            noise_table.device != dev or tuple(noise_table.shape) != (period * T, row) or \
            not noise_table.is_contiguous() or noise_table.data_ptr() % 16 != 0:
        raise ValueError(f"noise_table must be a contiguous, 16-byte aligned uint8 [{period * T}, "
                         f"{row}] tensor on {dev} (NoiseTable.to_device)")
    args = (ctypes.c_void_p(nominal_path.data_ptr()), BO, P, nominal_path.stride(0),
            nominal_path.stride(1), T, u0, count, n, ctypes.c_void_p(noise_table.data_ptr()), period,
            ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), ctypes.c_void_p(state.data_ptr()),
            ctypes.c_int32(1 if zero_first_step else 0),
            ctypes.c_void_p(ego_path.data_ptr()), ego_path.stride(1), ego_path.stride(0), O,
            ctypes.c_void_p(table.data_ptr()), D, ctypes.c_void_p(codes.data_ptr()),
            ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(status.data_ptr() if status is not None else None),
            ctypes.c_void_p(selected.data_ptr()), ctypes.c_void_p(_stream_handle(dev, stream)))
    launch = PreparedLaunch(lib.drcvar_sampled_halfspaces_f64_noise, args,
                            (nominal_path, ego_path, state, table, codes, noise_table, out, status,
                             selected))
    return launch, out, selected


def sampled_halfspaces_noise(nominal_path: torch.Tensor, ego_path: torch.Tensor, n_obstacles: int,
                             n_steps: int, n_samples: int, params: RiskTable, metric,
                             state: torch.Tensor, noise: NoiseTable, **kwargs
                             ) -> tuple[torch.Tensor, torch.Tensor]:
    """One ``drcvar_sampled_halfspaces_f64_noise`` launch (arguments:
    :func:`prepare_sampled_halfspaces_noise`): returns ``(out, selected)``."""
    launch, out, selected = prepare_sampled_halfspaces_noise(
        nominal_path, ego_path, n_obstacles, n_steps, n_samples, params, metric, state, noise,
        **kwargs)
    if out.numel() > 0:
        launch()
    return out, selected


def selected_views(selected: torch.Tensor, n_problems: int, n_obstacles: int):
    """``(h [B, O, T, 2], g [B, O, T])``: the solver's halfspace views of a whole-window
    ``selected [B O, T, 4]``, strided, no copy."""
    B, O = int(n_problems), int(n_obstacles)
    if selected.dim() != 3 or selected.shape[0] != B * O or selected.shape[2] != SELECTED_WIDTH:
        raise ValueError(f"selected must be [{B * O}, T, {SELECTED_WIDTH}], got {tuple(selected.shape)}")
    v = selected.view(B, O, selected.shape[1], SELECTED_WIDTH)
    return v[..., 0:2], v[..., 2]


def offsets_given_h(samples: torch.Tensor, h: torch.Tensor, params: RiskParams = RiskParams(),
                    out: torch.Tensor | None = None, stream=None,
                    status: torch.Tensor | None = None) -> torch.Tensor:
    """``cvar_halfspace`` / ``dr_cvar_halfspace`` for U units with given directions.

    samples [U, N, 2] float64 (device), h [U, 2] float64 (device) -> [U, 8] float64 (same columns;
    h echoed in columns 3..4).  ``status`` (optional int32 ``[U]``) receives the ``UNIT_*`` bits.
    """
    params.validate()
    _check_samples(samples, 3)
    U, N, _ = samples.shape
    _check_pairs(h, "h", U, samples.device)
    if out is None:
        out = torch.empty((U, OUT_WIDTH), dtype=torch.float64, device=samples.device)
    else:
        _check_out(out, (U, OUT_WIDTH), samples.device, "[U, 8]")
    if status is not None:
        _check_status(status, U, samples.device)
    if U == 0:
        return out
    lib = _native.lib()
    _native.check(lib.drcvar_offsets_given_h_f64_v2(
        ctypes.c_void_p(samples.data_ptr()), U, N, samples.stride(0), samples.stride(1),
        ctypes.c_void_p(h.data_ptr()), h.stride(0),
        params.robot_radius, params.obstacle_radius, params.alpha, params.delta, params.epsilon,
        ctypes.c_void_p(out.data_ptr()),
        ctypes.c_void_p(status.data_ptr() if status is not None else None),
        ctypes.c_void_p(_stream_handle(samples.device, stream))))
    return out
