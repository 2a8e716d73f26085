"""An all-host oracle of one control step of the receding-horizon loops (simulation/closed_loop.py:
RecedingHorizonFilter, RecedingHorizonBatch with ``linearize="reference"``).  A helper of
tests/test_closed_loop_oracle_host.py (CPU) and tests/test_closed_loop_oracle_gpu.py (GPU): plain
NumPy, never the product path.  It composes the three independent oracles the kernels are held to
one by one (oracle/philox_sampler.py, tests/halfspace_reference.py, oracle/mpc_qp.py) the way the
loop composes its three launches, and it imports neither the engine nor ``_native`` nor torch.

The step
--------
A :class:`LoopSpec` holds the loop's construction arguments as host arrays, always with a leading
problem dimension (the single loop is the batch of one problem with draw period 1), and the
arguments of ``reset(x0, step, stream_offset)``.  :func:`step` rebuilds step ``i`` (counted from
the reset) of problem ``b`` FROM A GIVEN STATE ``x0``:

* windows: rows ``clip(step + i + k, 0, P - 1)`` of problem b's nominal, reference and ego
  (``x_ref @ C.T``) paths, ``k < H`` (``k <= H`` for the state reference);
* samples: ``philox_sampler.sample_trajectories`` with the loop's seed and the stream words of
  ``(stream_offset + i) mod 2^64``; the counter is window-relative, problem b's obstacles sit at
  obstacle rows ``(b mod D) O .. + O`` of the draw (D the draw period, B for independent draws),
  and unit ``(o, t)`` takes the factor ``chol[b, o, t]``;
* record: ``halfspace_reference.reference`` on those samples with the problem's own (alpha, delta,
  epsilon) and its ego window; ``(h, g)`` are the columns :data:`METRIC_COLUMNS` names for the
  problem's metric (a restatement of ``core/mpc_filter.METRIC_COLUMNS``, compared with it by a CPU
  test);
* QP: ``mpc_qp.filter_trajectory`` from ``x0`` with the model's bounds; window step ``t``'s
  halfspaces constrain ``x[t + 1]``.

Re-anchoring: the GPU test passes the state the DEVICE logged for step i, bit for bit, so the
device's solver tolerance never compounds over steps and each step is an independent comparison.
:func:`free_run` instead feeds the oracle's own next state (plus the disturbance row) forward; the
CPU tests use it to certify the inputs and to measure what a wiring mistake does.

``mutate=`` plants one wiring mistake (:data:`MUTATIONS`) in the oracle: ``offset`` — the stream
offset of step 0 at every step; ``noise_row`` — the next problem's noise factors; ``route`` — the
next problem's route gives the ego window; ``metric`` — the next problem's metric; ``draw_period``
— the period ignored (with D < B every problem draws its own block b, with D = B every problem
draws block 0).  :func:`affected` says which problems a mutation can reach at all.

Record tolerance
----------------
The device draws its samples itself; they agree with the mirror's to ``SAMPLE_TOL`` = 1e-14 per
coordinate (tests/test_sampling.py, for factors up to 1).  ``halfspace_reference`` bounds the
kernel's error ON EQUAL SAMPLES (``Ref.bound*``); what a sample perturbation ``|dx_i|, |dy_i| <=
e`` adds follows from three Lipschitz constants, with ``|.|`` the Euclidean norm:

* the mean ``mu``: each coordinate moves by at most e, ``|d mu| <= sqrt(2) e``;
* a direction ``v / |v|``: ``|a/|a| - b/|b|| <= 2 |a - b| / max(|a|, |b|)``, so the mean direction
  (``v = mu``) moves by at most ``2 sqrt(2) e / |mu|`` and the halfspace direction (``v = mu -
  ego``, rho = |v|) by ``dh = 2 sqrt(2) e / rho``; ``g_mean = R_c - |mu|`` moves by at most
  ``sqrt(2) e``;
* the tail mean ``L = (sum_{j<m} d_(j) + (k - m) d_(m)) / k`` is the minimum over weights ``0 <=
  w_i <= 1 / k, sum w_i = 1`` of ``sum w_i d_i``, so it is 1-Lipschitz in ``max_i |d d_i|``, and a
  projection ``d_i = h . s_i`` moves by at most ``|h| sqrt(2) e + dh max_i |s_i|``.  The three
  offsets are ``L`` plus terms in ``|h| = 1``, so they move by that much.

:func:`record_tolerance` returns, per column, the reference's own bound plus this term at e =
``SAMPLE_TOL``; for the loops' scenarios the sum is about 1e-13, far below ``OFFSET_TOL`` = 1e-6,
which tests/test_closed_loop_oracle_host.py asserts together with the perturbation terms
themselves (a random +-e perturbation of the samples moves no column by more).
"""
import dataclasses

import numpy as np

import halfspace_reference as hr
from oracle import mpc_qp, philox_sampler

METRIC_COLUMNS = {"mean": (0, 2), "cvar": (3, 5), "dr_cvar": (3, 7)}    # (first h column, g column)
MUTATIONS = ("offset", "noise_row", "route", "metric", "draw_period")
SAMPLE_TOL = 1e-14
_SQRT2 = float(np.sqrt(2.0))


@dataclasses.dataclass(frozen=True)
class LoopSpec:
    """A loop's construction and reset arguments as host arrays (see :func:`loop_spec`)."""

    A: np.ndarray
    B: np.ndarray
    C: np.ndarray
    Q: np.ndarray
    R: np.ndarray
    u_bounds: tuple
    p_bounds: tuple
    horizon: int
    nominal: np.ndarray        # [Bn, O, P, 2]
    x_ref: np.ndarray          # [Bn, P, nx]
    u_ref: np.ndarray          # [Bn, P, nu]
    n_samples: int
    risk: np.ndarray           # [Bn, 3]: alpha, delta, epsilon
    radii: tuple               # (robot, obstacle)
    metrics: tuple             # Bn names
    chol: np.ndarray           # [Bn, O, H, 3]
    draw_period: int
    seed: int
    zero_first_step: bool
    disturbance: object        # [Bn, D, nx] or None
    step: int
    stream_offset: int

    @property
    def n_problems(self):
        return self.nominal.shape[0]

    @property
    def n_obstacles(self):
        return self.nominal.shape[1]

    @property
    def path_steps(self):
        return self.nominal.shape[2]

    @property
    def ego(self):
        """[Bn, P, 2], the path the halfspaces are taken about."""
        return self.x_ref @ self.C.T


def loop_spec(model, nominal, x_ref, u_ref, n_samples, *, horizon, chol, n_problems=1,
              alpha=0.2, delta=0.1, epsilon=0.15, radii=(0.3, 0.3), metric="dr_cvar",
              draw_period=None, seed=0, zero_first_step=True, disturbance=None, step=0,
              stream_offset=0):
    """``model``: a mapping with A, B, C, Q, R, u_bounds, p_bounds.  ``nominal`` is ``[O, P, 2]``
    or ``[B, O, P, 2]``, the reference paths ``[P, .]`` or ``[B, P, .]``, ``alpha`` / ``delta`` /
    ``epsilon`` scalars or ``[B]``, ``metric`` a name or B names, ``chol`` one factor ``(l00, l10,
    l11)`` or an array broadcastable to ``[B, O, H, 3]``, ``disturbance`` ``[D, nx]`` (one problem)
    or ``[B, D, nx]``.  ``draw_period=None`` is independent draws (D = B)."""
    Bn, H = int(n_problems), int(horizon)
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    nominal, x_ref, u_ref = f64(nominal), f64(x_ref), f64(u_ref)
    O, P = nominal.shape[-3], nominal.shape[-2]
    nominal = np.broadcast_to(nominal, (Bn, O, P, 2))
    x_ref = np.broadcast_to(x_ref, (Bn, P, x_ref.shape[-1]))
    u_ref = np.broadcast_to(u_ref, (Bn, P, u_ref.shape[-1]))
    risk = np.stack([np.broadcast_to(f64(v), (Bn,)) for v in (alpha, delta, epsilon)], axis=1)
    metrics = (metric,) * Bn if isinstance(metric, str) else tuple(metric)
    if len(metrics) != Bn or any(m not in METRIC_COLUMNS for m in metrics):
        raise ValueError(f"metric {metric!r} does not name {Bn} known metrics")
    if disturbance is not None:
        disturbance = f64(disturbance)
        disturbance = np.broadcast_to(disturbance, (Bn,) + disturbance.shape[-2:])
    D = Bn if draw_period is None else int(draw_period)
    if D < 1:
        raise ValueError(f"draw_period={draw_period} must be at least 1")
    return LoopSpec(f64(model["A"]), f64(model["B"]), f64(model["C"]), f64(model["Q"]), f64(model["R"]),
                    tuple(model["u_bounds"]), tuple(model["p_bounds"]), H, nominal, x_ref, u_ref,
                    int(n_samples), risk, (float(radii[0]), float(radii[1])), metrics,
                    np.broadcast_to(f64(chol), (Bn, O, H, 3)), D, int(seed), bool(zero_first_step),
                    disturbance, int(step), int(stream_offset))


def load_model(path):
    """The model of a tests/golden/mpc_*.npz file as :func:`loop_spec` takes it."""
    m = np.load(path, allow_pickle=False)
    return {"A": m["A"], "B": m["B"], "C": m["C"], "Q": m["Q"], "R": m["R"],
            "u_bounds": tuple(m["u_bounds"]), "p_bounds": tuple(m["p_bounds"])}


# ---------------------------------------------------------------------------------------------
# the pieces of one step
# ---------------------------------------------------------------------------------------------
def window_rows(spec, i, rows):
    """Path rows of step i's window: ``clip(step + i + k, 0, P - 1)``, ``k < rows``."""
    return np.clip(spec.step + int(i) + np.arange(rows), 0, spec.path_steps - 1)


def _next(spec, b):
    return (b + 1) % spec.n_problems


def draw_block(spec, b, mutate=None):
    """The obstacle block of the draw that problem b's units sit at."""
    if mutate == "draw_period":
        return b if spec.draw_period < spec.n_problems else 0
    return b % spec.draw_period


def affected(spec, mutation):
    """The problems a mutation can reach at all: those whose own row differs from the row the
    mutation reads instead (``offset`` reaches every problem, from step 1 on)."""
    Bn = spec.n_problems
    if mutation == "offset":
        return list(range(Bn))
    if mutation == "noise_row":
        return [b for b in range(Bn) if not np.array_equal(spec.chol[b], spec.chol[_next(spec, b)])]
    if mutation == "route":
        # (the ego enters the direction h and the offsets taken along it, never the mean halfspace
        # (hm, g_mean): a problem under the mean metric cannot see whose route gave the ego)
        ego = spec.ego
        return [b for b in range(Bn) if spec.metrics[b] != "mean"
                and not np.array_equal(ego[b], ego[_next(spec, b)])]
    if mutation == "metric":
        return [b for b in range(Bn)
                if METRIC_COLUMNS[spec.metrics[b]] != METRIC_COLUMNS[spec.metrics[_next(spec, b)]]]
    if mutation == "draw_period":
        return [b for b in range(Bn) if draw_block(spec, b) != draw_block(spec, b, mutation)]
    raise ValueError(mutation)


def samples(spec, i, b, mutate=None):
    """``[O, H, N, 2]``: the draws of problem b at step i."""
    O, H = spec.n_obstacles, spec.horizon
    window = spec.nominal[b][:, window_rows(spec, i, H)]                      # [O, H, 2]
    block = draw_block(spec, b, mutate)
    grid = np.zeros(((block + 1) * O, H, 2))       # (the rows before the block only place the counter)
    grid[block * O:] = window
    chol = np.zeros(((block + 1) * O, H, 3))
    chol[block * O:] = spec.chol[_next(spec, b) if mutate == "noise_row" else b]
    factor = tuple(chol[..., c].reshape(-1, 1) for c in range(3))           # one factor per unit
    offset = (spec.stream_offset + (0 if mutate == "offset" else int(i))) % 2 ** 64
    drawn = philox_sampler.sample_trajectories(grid, spec.n_samples, factor, spec.seed, offset,
                                               spec.zero_first_step)
    return np.ascontiguousarray(drawn[block * O:])


def ego_window(spec, i, b, mutate=None):
    """``[H, 2]``: the points step i's halfspaces of problem b are taken about."""
    return spec.ego[_next(spec, b) if mutate == "route" else b][window_rows(spec, i, spec.horizon)]


def record(spec, i, b, mutate=None, drawn=None):
    """``halfspace_reference.Ref`` of problem b's O H units at step i (unit ``o H + t``)."""
    O, H = spec.n_obstacles, spec.horizon
    if drawn is None:
        drawn = samples(spec, i, b, mutate)
    alpha, delta, epsilon = (float(v) for v in spec.risk[b])
    return hr.reference(drawn.reshape(O * H, spec.n_samples, 2),
                        ego=np.tile(ego_window(spec, i, b, mutate), (O, 1)), alpha=alpha, delta=delta,
                        epsilon=epsilon, rr=spec.radii[0], ro=spec.radii[1])


def halfspaces(spec, rec, b, mutate=None):
    """``[O, H, 3]`` = (h0, h1, g) under problem b's metric from a record ``[O H, 8]``."""
    ch, cg = METRIC_COLUMNS[spec.metrics[_next(spec, b) if mutate == "metric" else b]]
    r = np.asarray(rec).reshape(spec.n_obstacles, spec.horizon, 8)
    return np.concatenate([r[..., ch:ch + 2], r[..., cg:cg + 1]], axis=-1)


@dataclasses.dataclass
class StepAnswer:
    x: np.ndarray            # [H + 1, nx]
    u: np.ndarray            # [H, nu]
    status: str
    objective: float
    slacks: np.ndarray
    kkt: dict
    ref: object              # halfspace_reference.Ref of the step's units
    hs: np.ndarray           # [O, H, 3] the QP's halfspaces


def solve(spec, i, b, x0, hs):
    """``mpc_qp.filter_trajectory`` of problem b at step i from ``x0`` on halfspaces ``[O, H, 3]``."""
    H = spec.horizon
    return mpc_qp.filter_trajectory(spec.A, spec.B, spec.C, spec.Q, spec.R, H, x0,
                                    spec.x_ref[b][window_rows(spec, i, H + 1)],
                                    spec.u_ref[b][window_rows(spec, i, H)],
                                    [hs[:, t] for t in range(H)], spec.u_bounds, spec.p_bounds)


def step(spec, i, b, x0, mutate=None):
    """Step i of problem b from the state ``x0`` -> :class:`StepAnswer`."""
    ref = record(spec, i, b, mutate)
    hs = halfspaces(spec, ref.rec, b, mutate)
    x, u, info = solve(spec, i, b, x0, hs)
    return StepAnswer(x, u, info["status"], info.get("objective", np.nan), info.get("slacks"),
                      info.get("kkt"), ref, hs)


def sensitivity(spec, i, b, x0, answer, shift=1e-9):
    """Largest ``|du| / |dg|`` of a step, measured with every offset g shifted by ``shift``."""
    hs = answer.hs.copy()
    hs[..., 2] += shift
    _, u, _ = solve(spec, i, b, x0, hs)
    return float(np.abs(u - answer.u).max() / shift)


def free_run(spec, n_steps, b, x0, mutate=None, until=None):
    """Problem b's loop with the oracle feeding its own next state (+ the disturbance row):
    ``(states [n + 1, nx], answers)``.  ``until(i, answer)`` true ends the run after step i."""
    x = np.array(x0, dtype=np.float64)
    states, answers = [x.copy()], []
    for i in range(int(n_steps)):
        a = step(spec, i, b, x, mutate)
        answers.append(a)
        x = a.x[1] + spec.disturbance[b, i] if spec.disturbance is not None else a.x[1].copy()
        states.append(x.copy())
        if until is not None and until(i, a):
            break
    return np.stack(states), answers


# ---------------------------------------------------------------------------------------------
# record tolerance
# ---------------------------------------------------------------------------------------------
def perturbation_terms(drawn, ego, e=SAMPLE_TOL):
    """What a sample perturbation of at most ``e`` per coordinate moves each record column by
    (module docstring): ``[U, 8]`` for ``drawn [U, N, 2]`` and ``ego [U, 2]``."""
    s = np.asarray(drawn, dtype=np.float64)
    mu = s.mean(axis=1)
    mu_norm = np.hypot(mu[:, 0], mu[:, 1])
    rho = np.hypot(*(mu - np.asarray(ego, dtype=np.float64)).T)
    if not (np.all(mu_norm > 1e-6) and np.all(rho > 1e-6)):
        raise ValueError("a unit whose mean or separation is (nearly) zero has no Lipschitz direction")
    reach = np.hypot(s[..., 0], s[..., 1]).max(axis=1)
    d_hm, d_h = 2 * _SQRT2 * e / mu_norm, 2 * _SQRT2 * e / rho
    d_g = _SQRT2 * e + d_h * reach
    return np.stack([d_hm, d_hm, np.full_like(d_hm, _SQRT2 * e), d_h, d_h, d_g, d_g, d_g], axis=1)


def reference_bounds(ref):
    """``[U, 8]``: halfspace_reference's own bound of every record column."""
    return np.stack([ref.bound_hm, ref.bound_hm, ref.bound_gm, ref.bound_h, ref.bound_h, ref.bound,
                     ref.bound, ref.bound], axis=1)


def record_tolerance(ref, drawn, ego):
    """``[U, 8]``: what a device record may differ from ``ref.rec`` by, column by column — the
    reference's bound on equal samples plus the effect of samples that differ by SAMPLE_TOL."""
    return reference_bounds(ref) + perturbation_terms(drawn, ego)


def step_record(spec, i, b):
    """``(ref, tolerance [O H, 8])`` of problem b's units at step i."""
    O, H = spec.n_obstacles, spec.horizon
    drawn = samples(spec, i, b)
    ref = record(spec, i, b, drawn=drawn)
    tol = record_tolerance(ref, drawn.reshape(O * H, spec.n_samples, 2), np.tile(ego_window(spec, i, b), (O, 1)))
    return ref, tol


def rollout_ld(A, B, x0, u):
    """``x[t + 1] = A x[t] + B u[t]`` in np.longdouble."""
    LD = np.longdouble
    A, B, u = np.asarray(A).astype(LD), np.asarray(B).astype(LD), np.asarray(u).astype(LD)
    x = [np.asarray(x0).astype(LD)]
    for t in range(u.shape[0]):
        x.append(A @ x[-1] + B @ u[t])
    return np.stack(x)
