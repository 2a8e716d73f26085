"""Monte Carlo out-of-sample collision evaluation: how often does each filtered trajectory collide
when the obstacles do not follow the Gaussian samples its halfspaces were fitted to?

Reference: ``main.py:128-138`` answers with ONE Laplace realisation per obstacle
(``simulation/obstacles.py:79-113``) and the per-step clearance against it
(``simulation/environment.py:108-140``).  Two paths:

* device (``drcvar_min_clearance_f64``, ``include/drcvar_sampling.h``) — M realisations drawn by
  Philox4x32-10 and reduced to one minimum clearance per trajectory and realisation inside the
  kernel; no realisation is ever stored.  All trajectories of a call see the same draws (common
  random numbers), so mean, CVaR and DR-CVaR trajectories are compared on identical obstacles.
* host — the reference's own procedure repeated M times on the global ``np.random`` stream
  (``generate_laplace_realization`` per obstacle in order, then ``compute_distance_to_collision``):
  a seeded run equals what the reference's code produces.  The parity path and the CPU baseline.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _native
from ..simulation.obstacles import NOISE_COV, generate_laplace_realization
from . import metrics

MAX_TRAJECTORIES = 8          # trajectories one launch evaluates (include/drcvar_sampling.h)
NOISE_KINDS = {"gaussian": 0, "laplace": 1}


def _noise_params(noise, noise_cov):
    """(kind, p0, p1, p2) of the C entry: Laplace scales sqrt(diag(cov) / 2) (obstacles.py:100) or
    the lower Cholesky factor of the Gaussian's covariance."""
    if noise not in NOISE_KINDS:
        raise ValueError(f"noise must be 'laplace' or 'gaussian', not {noise!r}")
    cov = np.asarray(noise_cov, dtype=np.float64).reshape(2, 2)
    if noise == "laplace":
        scale = np.sqrt(np.diag(cov) / 2)
        return 1, float(scale[0]), float(scale[1]), 0.0
    L = np.linalg.cholesky(cov)
    return 0, float(L[0, 0]), float(L[1, 0]), float(L[1, 1])


def _check_positions(name, x, dims):
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise ValueError(f"{name} must be a device tensor (the evaluation kernel has no CPU path)")
    if x.dtype != torch.float64 or x.dim() != 3 or x.shape[2] != 2 or x.stride(2) != 1:
        raise ValueError(f"{name} must be float64 {dims} with adjacent coordinates")


def min_clearance_device(ego, nominal, n_realizations, *, noise="laplace", noise_cov=NOISE_COV,
                         robot_radius, obstacle_radius, seed=0, stream_offset=0,
                         first_realization=0, zero_first_step=True, step_hits=False, step_splits=0,
                         out=None, stream=None):
    """Minimum clearance ``[K, M]`` of the trajectories ``ego`` ``[K, T, 2]`` against ``M`` noise
    realisations ``first_realization .. first_realization + M - 1`` of the obstacles' ``nominal``
    ``[O, T, 2]`` paths (float64 device tensors, any strides with adjacent coordinates).

    ``out[k, m] = min over (o, t) of |ego[k, t] - (nominal[o, t] + noise[m, o, t])| - (robot_radius +
    obstacle_radius)``.  The noise of realisation m depends on (seed, stream_offset, m, o, t, O, T)
    only: a window of a longer run, a subset of the trajectories or another ``step_splits`` gives
    the same bits.  With ``step_hits=True`` also returns ``[K, T]`` int64, the number of
    realisations in collision at each step.  ``out`` may be any float64 ``[K, M]`` view with
    adjacent realisations.  Non-finite positions follow IEEE 754: ``out[k, m]`` is NaN exactly when
    a squared distance entering it is NaN, and such a step counts nothing; nothing else changes.
    """
    _check_positions("ego", ego, "[K, T, 2]")
    _check_positions("nominal", nominal, "[O, T, 2]")
    if nominal.device != ego.device:
        raise ValueError("ego and nominal must be on the same device")
    K, T, _ = ego.shape
    O = nominal.shape[0]
    if nominal.shape[1] != T:
        raise ValueError(f"ego has {T} steps, nominal {nominal.shape[1]}")
    if not 1 <= K <= MAX_TRAJECTORIES:
        raise ValueError(f"between 1 and {MAX_TRAJECTORIES} trajectories per call, not {K}")
    M, first = int(n_realizations), int(first_realization)
    if M < 0 or first < 0:
        raise ValueError("n_realizations and first_realization must not be negative")
    kind, p0, p1, p2 = _noise_params(noise, noise_cov)
    if out is None:
        out = torch.empty((K, M), dtype=torch.float64, device=ego.device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (K, M) or \
            out.dtype != torch.float64 or out.device != ego.device or (M > 1 and out.stride(1) != 1):
        raise ValueError("out must be a float64 [K, M] device view with adjacent realisations")
    # the call sets step_hits, it does not accumulate into it
    hits = torch.empty((K, T), dtype=torch.int64, device=ego.device) if step_hits else None
    s = stream if stream is not None else torch.cuda.current_stream(ego.device)
    _native.check(_native.lib().drcvar_min_clearance_f64_ex(
        ctypes.c_void_p(ego.data_ptr()), K, ego.stride(0), ego.stride(1),
        ctypes.c_void_p(nominal.data_ptr()), O, T, nominal.stride(0), nominal.stride(1),
        kind, p0, p1, p2, float(robot_radius) + float(obstacle_radius), first, M,
        ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), ctypes.c_uint64(int(stream_offset) & (2 ** 64 - 1)),
        1 if zero_first_step else 0, ctypes.c_void_p(out.data_ptr()), out.stride(0),
        ctypes.c_void_p(hits.data_ptr()) if step_hits else None, int(step_splits),
        ctypes.c_void_p(int(s.cuda_stream))))
    return (out, hits) if step_hits else out


# ---- the loop form: the current state of B loops per launch (include/drcvar_loop_eval.h) ----------
LOOP_EVAL_BLOCK = 256            # realisations one workgroup covers per realisation per thread
LOOP_EVAL_RULE_PER_THREAD = 8    # the most realisations per thread the library's rule chooses
LOOP_EVAL_MAX_PER_THREAD = 64    # ... and the most ``realizations_per_thread`` may ask for
MAX_LOOP_STATES = 8


def _loop_eval_check(x0, c_out, nominal_path, n_obstacles, state, min_d2, step_hits, log_rows):
    """The buffers of a loop-evaluation launch against each other (host only: shapes, dtypes,
    strides, devices).  Returns ``(B, nx, O, P, M, c_out as a contiguous host array)``."""
    if not isinstance(x0, torch.Tensor) or x0.dtype != torch.float64 or x0.dim() != 2 or \
            not x0.is_contiguous():
        raise ValueError("x0 must be a contiguous float64 [B, nx] tensor")
    B, nx = x0.shape
    if B < 1 or not 1 <= nx <= MAX_LOOP_STATES:
        raise ValueError(f"x0 is [B, nx] with B >= 1 and nx in 1..{MAX_LOOP_STATES}, got {tuple(x0.shape)}")
    c = np.ascontiguousarray(np.asarray(c_out, dtype=np.float64))
    if c.shape != (2, nx):
        raise ValueError(f"c_out must be [2, {nx}] (the model's position rows), got {c.shape}")
    O, rows = int(n_obstacles), int(log_rows)
    if O < 1 or rows < 0:
        raise ValueError("n_obstacles must be at least 1 and log_rows must not be negative")
    t = nominal_path
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != 3 or \
            t.shape[0] != B * O or t.shape[1] < 1 or t.shape[2] != 2 or t.stride(2) != 1:
        raise ValueError(f"nominal_path must be float64 [B O = {B * O}, P, 2] with adjacent coordinates")
    if not isinstance(state, torch.Tensor) or state.dtype != torch.int64 or state.numel() != 2 * B or \
            not state.is_contiguous() or state.shape[-1] != 2:
        raise ValueError(f"state must be a contiguous int64 [B = {B}, 2] tensor ([stream_offset, step])")
    if not isinstance(min_d2, torch.Tensor) or min_d2.dtype != torch.float64 or min_d2.dim() != 2 or \
            min_d2.shape[0] != B or (min_d2.shape[1] > 1 and min_d2.stride(1) != 1):
        raise ValueError(f"min_d2 must be a float64 [B = {B}, M] view with adjacent realisations")
    if step_hits is not None and (not isinstance(step_hits, torch.Tensor) or
                                  step_hits.dtype != torch.int64 or not step_hits.is_contiguous() or
                                  tuple(step_hits.shape) != (B, rows + 1)):
        raise ValueError(f"step_hits must be a contiguous int64 [B = {B}, log_rows + 1 = {rows + 1}] tensor")
    for name, buf in (("nominal_path", t), ("state", state), ("min_d2", min_d2), ("step_hits", step_hits)):
        if buf is not None and buf.device != x0.device:
            raise ValueError(f"{name} must be on x0's device {x0.device}, got {buf.device}")
    if x0.device.type != "cuda":
        raise ValueError("the buffers must be device tensors (the evaluation kernel has no CPU path)")
    return B, nx, O, t.shape[1], min_d2.shape[1], c


def prepare_loop_clearance_step(x0, c_out, nominal_path, n_obstacles, state, min_d2, step_hits=None, *,
                                step_begin=0, log_rows=0, noise_steps=None, noise="laplace",
                                noise_cov=NOISE_COV, robot_radius, obstacle_radius, seed=0,
                                eval_offset=0, problem_offset_stride=1, zero_first_step=True,
                                realizations_per_thread=0, stream=None):
    """Freeze one ``drcvar_loop_clearance_f64_ex`` call (``include/drcvar_loop_eval.h``) on
    ``stream``: every call of the returned launch evaluates the state ``x0 [B, nx]`` each of B
    loops is in NOW, at its path row ``state[b, 1]``, against ``M`` noise realisations of its
    obstacles ``nominal_path [B O, P, 2]``, and accumulates ``min_d2 [B, M]`` (running minimum of
    the squared distance; fill with +inf first) and ``step_hits [B, log_rows + 1]`` (collisions
    per step since ``step_begin``; fill with 0 first; optional).  Capturable: nothing that changes
    from step to step is frozen.  ``noise_steps`` (default P) is the T of the
    ``min_clearance_device`` call whose draws these are: problem b at row s sees bit for bit that
    call's noise at step s with ``stream_offset = eval_offset + b problem_offset_stride``."""
    B, nx, O, P, M, c = _loop_eval_check(x0, c_out, nominal_path, n_obstacles, state, min_d2,
                                         step_hits, log_rows)
    kind, p0, p1, p2 = _noise_params(noise, noise_cov)
    Tn = P if noise_steps is None else int(noise_steps)
    per = int(realizations_per_thread)
    if Tn < 0 or not 0 <= per <= LOOP_EVAL_MAX_PER_THREAD:
        raise ValueError(f"noise_steps must not be negative and realizations_per_thread must be in "
                         f"0..{LOOP_EVAL_MAX_PER_THREAD}")
    from .. import engine
    s = stream if stream is not None else torch.cuda.current_stream(x0.device)
    vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
    mask = 2 ** 64 - 1
    return engine.PreparedLaunch(_native.eval_lib().drcvar_loop_clearance_f64_ex, (
        B, vp(x0.data_ptr()), i32(nx), vp(c.ctypes.data), vp(nominal_path.data_ptr()), O, P,
        nominal_path.stride(0), nominal_path.stride(1), vp(state.data_ptr()), int(step_begin),
        int(log_rows), Tn, i32(kind), p0, p1, p2, float(robot_radius) + float(obstacle_radius), M,
        u64(int(seed) & mask), u64(int(eval_offset) & mask), u64(int(problem_offset_stride) & mask),
        i32(1 if zero_first_step else 0), vp(min_d2.data_ptr()), min_d2.stride(0),
        vp(step_hits.data_ptr() if step_hits is not None else None), i32(per),
        vp(int(s.cuda_stream))), (x0, c, nominal_path, state, min_d2, step_hits))


def loop_clearance_step(x0, c_out, nominal_path, n_obstacles, state, min_d2, step_hits=None, **kw):
    """One checked ``drcvar_loop_clearance_f64`` launch: :func:`prepare_loop_clearance_step`'s
    arguments, issued once.  Returns ``(min_d2, step_hits)``, the accumulated buffers."""
    prepare_loop_clearance_step(x0, c_out, nominal_path, n_obstacles, state, min_d2, step_hits, **kw)()
    return min_d2, step_hits


def laplace_realizations_host(nominal_trajectories, n_realizations, noise_cov=NOISE_COV):
    """``n_realizations`` lists of one Laplace realisation per obstacle, drawn as the reference
    draws them (main.py:61 via obstacles.py:79-113): obstacles in order, on the global
    ``np.random`` stream."""
    return [[generate_laplace_realization(np.asarray(nom, dtype=np.float64), noise_cov)
             for nom in nominal_trajectories] for _ in range(int(n_realizations))]


def _as_states(tr):
    """A trajectory as ``[T, 4]`` states: positions ``[T, 2]`` get zero velocities (C picks the
    positions back out exactly)."""
    tr = np.asarray(tr, dtype=np.float64)
    if tr.ndim != 2 or tr.shape[1] not in (2, 4):
        raise ValueError("a trajectory is [T, 4] states or [T, 2] positions")
    return tr if tr.shape[1] == 4 else np.hstack([tr, np.zeros_like(tr)])


def run_monte_carlo_simulation(env, trajectories, nominal_trajectories, n_realizations,
                               noise="laplace", backend="device", seed=0):
    """Out-of-sample evaluation of every trajectory in ``trajectories`` (``name -> [T, 4]`` states
    or ``[T, 2]`` positions, e.g. reference / mean / cvar / dr_cvar as in main.py:129-138) against
    ``n_realizations`` noise realisations of the obstacles' nominal paths.

    Returns ``name -> {"min_distances": [M], "metrics": safety_metrics(min_distances),
    "step_collision_rate": [n_steps], "step_hits": [n_steps]}`` with
    ``n_steps = min(len(trajectory), len(nominal[0]))`` over all trajectories (environment.py:119).
    ``backend="device"``: device tensors, all trajectories on the same draws (Philox key ``seed``).
    ``backend="host"``: NumPy arrays by the reference's procedure after ``np.random.seed(seed)``
    (``seed=None`` continues the stream), Laplace noise only; adds ``"step_distances"`` ``[M, n_steps]``.
    """
    names = list(trajectories)
    states = [_as_states(trajectories[n]) for n in names]
    nominal = [np.asarray(nom, dtype=np.float64) for nom in nominal_trajectories]
    M = int(n_realizations)
    if not names or not nominal:
        raise ValueError("at least one trajectory and one obstacle")
    n_steps = min(min(len(s) for s in states), len(nominal[0]))
    radii = dict(robot_radius=env.ROBOT_RADIUS, obstacle_radius=env.OBSTACLE_RADIUS)
    result = {}
    if backend == "host":
        if noise != "laplace":
            raise ValueError("the host backend is the reference's procedure: Laplace noise only")
        if seed is not None:
            np.random.seed(seed)
        dist = {n: np.empty((M, n_steps)) for n in names}
        for m, realization in enumerate(laplace_realizations_host(nominal, M)):
            for n, s in zip(names, states):
                dist[n][m] = env.compute_distance_to_collision(s[:n_steps], realization)
        for n in names:
            mins = dist[n].min(axis=1) if n_steps else np.full(M, np.inf)
            step_hits = (dist[n] < 0).sum(axis=0)
            result[n] = {"min_distances": mins, "metrics": metrics.safety_metrics(mins),
                         "step_collision_rate": step_hits / M, "step_hits": step_hits,
                         "step_distances": dist[n]}
        return result
    if backend != "device":
        raise ValueError(f"backend must be 'device' or 'host', not {backend!r}")
    from ..core import risk_metrics
    dev = risk_metrics.device()
    ego = np.stack([s[:n_steps] @ env.C.T for s in states])                  # environment.py:121
    ego_d = torch.as_tensor(np.ascontiguousarray(ego)).to(dev)
    nom_d = torch.as_tensor(np.ascontiguousarray(np.stack([nom[:n_steps] for nom in nominal]))).to(dev)
    for k0 in range(0, len(names), MAX_TRAJECTORIES):     # the same draws for every group of 8
        clr, hits = min_clearance_device(ego_d[k0:k0 + MAX_TRAJECTORIES], nom_d, M, noise=noise,
                                         seed=seed, step_hits=True, **radii)
        # a tensor divisor: dividing by a Python number multiplies by its rounded reciprocal
        rate = hits.to(torch.float64) / torch.full((), float(M), dtype=torch.float64, device=dev)
        for j, n in enumerate(names[k0:k0 + MAX_TRAJECTORIES]):
            result[n] = {"min_distances": clr[j], "metrics": metrics.safety_metrics(clr[j]),
                         "step_collision_rate": rate[j], "step_hits": hits[j]}
    return result
