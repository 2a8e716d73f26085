"""GPU: drcvar_loop_clearance_f64 alone (csrc/drcvar_clearance.hip with DRCVAR_LOOP_EVAL_LIBRARY,
include/drcvar_loop_eval.h, through evaluation/monte_carlo.py), driven by a scripted sequence of
states: the test writes x0 and state itself, no solver runs.

A case is a chain of 6 launches; problem b is at path row base[b] + r in launch r, with new
positions every launch, so one launch holds problems at different steps: evaluated ones (log row
i = log_rows included), and ones left alone (i = log_rows + 1, s = T_n, s < 0, s < step_begin).
Checked: sqrt(min_d2) - R against tests/loop_clearance_mirror.py at atol 1e-13 (the bound
tests/test_monte_carlo_gpu.py derives for the same draws at distances <= 30 and noise scales <= 1;
positions here lie in [-2, 2]), step_hits exactly (the mirror's margin |min_o d^2 - R^2| >= 1e-9 is
asserted), the rows of problems left alone byte for byte, guard words around both outputs, the
inputs unchanged; then bit for bit against the existing kernel (min_clearance_device, K = 1 per
problem, far-padded rows), and across realisations-per-thread settings.  Two further chains carry
a NaN (a state at one launch; an obstacle's nominal row): the running minimum takes it and keeps it,
that launch counts nothing for the realisations it touches, the other problems keep their bytes
(include/drcvar_loop_eval.h).
"""
import numpy as np
import pytest

import loop_clearance_mirror as lm
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.evaluation import monte_carlo as mc

pytestmark = pytest.mark.gpu

SEED = 2 ** 40 + 9
LAPLACE_COV = np.diag([2 * 0.3 ** 2, 2 * 0.7 ** 2])           # scales (0.3, 0.7)
GAUSS_COV = np.array([[0.25, 0.10], [0.10, 0.20]])            # L = (0.5, 0.2, 0.4)
LAUNCHES, P = 6, 5
ABOVE_ONE_WORKGROUP = mc.LOOP_EVAL_RULE_PER_THREAD * mc.LOOP_EVAL_BLOCK + 1     # 4097
# problem b's path row in launch 0 (then + 1 per launch)
BASES = [0, 1, -2, 3, 2]

# name: M, O, B, nx, T_n, noise, stride, eval_offset, zero_first, hits, (step_begin, log_rows), R
CASES = {
    "m1": (1, 1, 1, 2, 1, "laplace", 1, 0, True, True, (0, 10), 1.0),
    "m1_noisy_first": (1, 1, 1, 2, 1, "gaussian", 1, 3, False, True, (0, 10), 1.0),
    "m63": (63, 3, 2, 4, 7, "gaussian", 1, 2 ** 32 - 1, False, True, (1, 4), 1.0),
    "m64_no_hits": (64, 1, 5, 8, 7, "laplace", 0, 2 ** 64 - 1, True, False, (0, 10), 1.0),
    "m65_wrap": (65, 3, 2, 4, 7, "laplace", 1, 2 ** 64 - 1, False, True, (0, 10), 1.0),
    "m257": (257, 3, 5, 4, 7, "gaussian", 0, 2 ** 32 - 1, True, True, (1, 4), 1.0),
    "m257_carry": (257, 1, 5, 8, 7, "laplace", 1, 2 ** 32 - 1, True, True, (1, 4), 1.0),
    "above_one_workgroup": (ABOVE_ONE_WORKGROUP, 3, 2, 2, 7, "laplace", 1, 5, True, True, (0, 10), 1.0),
    "all_collide": (130, 3, 2, 4, 7, "laplace", 1, 7, True, True, (0, 10), 50.0),
    "none_collide": (130, 3, 2, 4, 7, "gaussian", 1, 7, False, True, (0, 10), 0.0),
}
# The chains with a NaN: (the case above they copy: the same shape, so script() seeds the same
# inputs; the problem that meets the NaN; the launch at which it does; what is overwritten:
# ("x0", state) at that launch only, or ("nominal", obstacle, path row), a whole row for all launches)
POISON = {
    "m65_wrap_nan_state": ("m65_wrap", 1, 2, ("x0", 3)),           # state nx - 1 is selected (ego x)
    "m257_nan_nominal": ("m257", 1, 2, ("nominal", 2, 3)),         # problem 1 is at row 3 in launch 2
}
CLEAN = list(CASES)
CASES.update({name: CASES[poison[0]] for name, poison in POISON.items()})


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def params_of(noise):
    cov = LAPLACE_COV if noise == "laplace" else GAUSS_COV
    kind, p0, p1, p2 = mc._noise_params(noise, cov)
    return cov, ((p0, p1) if kind == 1 else (p0, p1, p2))


def script(name):
    """The case's inputs (seeded by its shape): c_out, a selector that picks states nx - 1 and 0,
    the paths, and per launch the states x0 [B, nx] (positions in [-2, 2], the other states large)
    and the path rows."""
    M, O, B, nx, Tn = CASES[name][:5]
    rng = np.random.default_rng(1000 + M + 10 * O + 100 * B + nx + Tn)
    c_out = np.zeros((2, nx))
    c_out[0, nx - 1] = 1.0
    c_out[1, 0] = 1.0
    nominal = rng.uniform(-2, 2, size=(B * O, P, 2))
    x0 = rng.uniform(-1e3, 1e3, size=(LAUNCHES, B, nx))
    x0[:, :, nx - 1] = rng.uniform(-2, 2, size=(LAUNCHES, B))
    x0[:, :, 0] = rng.uniform(-2, 2, size=(LAUNCHES, B))
    steps = np.array([[BASES[b] + r for b in range(B)] for r in range(LAUNCHES)], dtype=np.int64)
    if name in POISON:
        _, problem, launch_at, what = POISON[name]
        if what[0] == "x0":
            x0[launch_at, problem, what[1]] = np.nan
        else:
            nominal[problem * O + what[1], what[2]] = np.nan
    return c_out, nominal, x0, steps


def mirror_chain(name, trace=None):
    """(min_d2 [B, M], step_hits [B, rows] or None, margin, log rows per launch and problem) of the
    whole chain, from min_d2 = +inf and step_hits = 7.  ``trace``: a list that receives (min_d2,
    step_hits) as they stand after each launch."""
    M, O, B, nx, Tn, noise, stride, offset, zero_first, with_hits, (begin, rows), R = CASES[name]
    c_out, nominal, x0, steps = script(name)
    min_d2 = np.full((B, M), np.inf)
    hits = np.full((B, rows + 1), 7, dtype=np.int64) if with_hits else None
    margin, visited = np.inf, []
    for r in range(LAUNCHES):
        m, i = lm.launch(x0[r], c_out, nominal, O, steps[r], min_d2, hits, step_begin=begin,
                         log_rows=rows, noise_steps=Tn, kind=noise, params=params_of(noise)[1],
                         combined_radius=R, seed=SEED, eval_offset=offset, stride=stride,
                         zero_first_step=zero_first)
        margin = min(margin, m)
        visited.append(i)
        if trace is not None:
            trace.append((min_d2.copy(), hits.copy() if with_hits else None))
    return min_d2, hits, margin, visited


def device_chain(dev, name, per_thread=0, trace=None):
    """The chain on the device; returns (min_d2, step_hits) as NumPy arrays after checking the
    guard words, the inputs, and after every launch the rows of the problems left alone.
    ``trace``: a list that receives (min_d2, step_hits) as NumPy arrays after each launch."""
    import torch
    M, O, B, nx, Tn, noise, stride, offset, zero_first, with_hits, (begin, rows), R = CASES[name]
    c_out, nominal, x0, steps = script(name)
    visited = mirror_chain(name)[3]
    nom_base = torch.full((B * O, P + 3, 2), -7.0, dtype=torch.float64, device=dev)
    nom_d = nom_base[:, 1:P + 1]                                           # a strided view
    nom_d.copy_(torch.from_numpy(nominal))
    out_base = torch.full((B + 2, M + 5), 123.0, dtype=torch.float64, device=dev)
    min_d2 = out_base[1:B + 1, :M]
    min_d2.fill_(float("inf"))
    hit_base = torch.full((B * (rows + 1) + 4,), -5, dtype=torch.int64, device=dev)
    hits = hit_base[2:-2].view(B, rows + 1) if with_hits else None
    if with_hits:
        hits.fill_(7)
    x0_d = torch.zeros((B, nx), dtype=torch.float64, device=dev)
    state = torch.zeros((B, 2), dtype=torch.int64, device=dev)
    launch = mc.prepare_loop_clearance_step(
        x0_d, c_out, nom_d, O, state, min_d2, hits, step_begin=begin, log_rows=rows, noise_steps=Tn,
        noise=noise, noise_cov=params_of(noise)[0], robot_radius=0.55 * R, obstacle_radius=0.45 * R,
        seed=SEED, eval_offset=offset, problem_offset_stride=stride, zero_first_step=zero_first,
        realizations_per_thread=per_thread)
    for r in range(LAUNCHES):
        x0_d.copy_(torch.from_numpy(x0[r]))
        state[:, 1].copy_(torch.from_numpy(steps[r]))
        state[:, 0].fill_(-r - 1)                                          # never read
        before = (min_d2.clone(), hits.clone() if with_hits else None, x0_d.clone(), state.clone())
        launch()
        alone = [b for b in range(B) if visited[r][b] is None]
        assert torch.equal(min_d2[alone].view(torch.int64), before[0][alone].view(torch.int64)), (r, alone)
        if with_hits:
            assert torch.equal(hits[alone], before[1][alone]), (r, alone)
        assert torch.equal(x0_d.view(torch.int64), before[2].view(torch.int64))   # (NaN included)
        assert torch.equal(state, before[3])
        if trace is not None:
            trace.append((min_d2.cpu().numpy(), hits.cpu().numpy() if with_hits else None))
    out = out_base.cpu().numpy()
    guard = np.ones(out.shape, dtype=bool)
    guard[1:B + 1, :M] = False
    assert np.all(out[guard] == 123.0)
    assert hit_base[:2].tolist() == [-5, -5] and hit_base[-2:].tolist() == [-5, -5]
    assert nom_d.cpu().numpy().tobytes() == nominal.tobytes() and bool(torch.all(nom_base[:, 0] == -7.0))
    return min_d2.cpu().numpy(), hits.cpu().numpy() if with_hits else None


def clearance(d2, R):
    return np.sqrt(d2) - R


@pytest.mark.parametrize("name", CLEAN)
def test_chain_matches_mirror(dev, name):
    M, O, B = CASES[name][:3]
    R = CASES[name][-1]
    want, want_hits, margin, visited = mirror_chain(name)
    assert margin >= 1e-9
    got, hits = device_chain(dev, name)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and not np.isnan(want).any()
    assert np.array_equal(np.isinf(got), np.isinf(want))
    seen = np.isfinite(want)
    assert seen.any()
    err = np.max(np.abs(clearance(got[seen], R) - clearance(want[seen], R)))
    print(f"{name}: max |kernel - mirror| = {err:.3e}, margin {margin:.2e}")
    assert err <= 1e-13
    if want_hits is not None:
        np.testing.assert_array_equal(hits, want_hits)
        counted = want_hits - 7
        if name == "all_collide":      # exactly M per evaluated state: no lane past M counts
            rows = sorted({(b, i) for row in visited for b, i in enumerate(row) if i is not None})
            assert all(counted[b, i] == M for b, i in rows) and counted.sum() == M * len(rows)
        if name == "none_collide":
            assert counted.sum() == 0


@pytest.mark.parametrize("name", ["m63", "m64_no_hits", "m65_wrap", "m257", "above_one_workgroup",
                                  "all_collide"])
def test_chain_matches_the_existing_kernel_bitwise(dev, name):
    """Per problem one min_clearance_device call (K = 1, T = T_n, the problem's stream offset) on an
    ego whose visited rows hold the chain's positions and whose other rows lie 1e3 away from every
    obstacle: the same clearances and hit rows, bit for bit."""
    import torch
    M, O, B, nx, Tn, noise, stride, offset, zero_first, with_hits, (begin, rows), R = CASES[name]
    c_out, nominal, x0, steps = script(name)
    visited = mirror_chain(name)[3]
    got, hits = device_chain(dev, name)
    path_rows = np.minimum(np.arange(Tn), P - 1)
    for b in range(B):
        nom = nominal[b * O:(b + 1) * O][:, path_rows]                      # [O, T_n, 2]
        ego = np.stack((nom[..., 0].max(axis=0) + 1e3, nom[0, :, 1]), axis=1)
        seen = [(int(steps[r][b]), visited[r][b]) for r in range(LAUNCHES) if visited[r][b] is not None]
        for r in range(LAUNCHES):
            if visited[r][b] is not None:
                ego[steps[r][b]] = lm.ego_of(c_out, x0[r][b])
        if not seen:
            assert np.all(np.isinf(got[b]))
            continue
        clr, h = mc.min_clearance_device(
            torch.from_numpy(ego[None]).to(dev), torch.from_numpy(nom).to(dev), M, noise=noise,
            noise_cov=params_of(noise)[0], robot_radius=0.55 * R, obstacle_radius=0.45 * R, seed=SEED,
            stream_offset=(offset + b * stride) & lm.MASK64, zero_first_step=zero_first, step_hits=True)
        assert np.array_equal(clearance(got[b], 0.55 * R + 0.45 * R), clr[0].cpu().numpy()), b
        if with_hits:
            h = h[0].cpu().numpy()
            for s, i in seen:
                assert hits[b, i] - 7 == h[s], (b, s, i)


@pytest.mark.parametrize("name", ["m65_wrap", "m257", "above_one_workgroup"])
def test_geometry_independence(dev, name):
    base, base_hits = device_chain(dev, name)
    for per in (1, 3, mc.LOOP_EVAL_RULE_PER_THREAD, mc.LOOP_EVAL_MAX_PER_THREAD):
        got, hits = device_chain(dev, name, per_thread=per)
        assert got.tobytes() == base.tobytes(), per
        assert np.array_equal(hits, base_hits), per


@pytest.mark.parametrize("per_thread", [0, 1, 3])
@pytest.mark.parametrize("name", list(POISON))
def test_nan_is_taken_kept_and_not_counted(dev, name, per_thread):
    """After every launch of a chain with a NaN, against the mirror (np.minimum and ndarray.min
    propagate NaN) and against the clean chain under the same geometry: the same elements are NaN
    (the poisoned problem's row from the launch that meets the NaN to the end), the others agree
    at atol 1e-13 in clearance, step_hits are the mirror's exactly (the poisoned launch adds
    nothing; later launches count again), and the other problems' bytes are the clean chain's.
    The margin is the clean case's: the NaN removes d^2 values from the mirror's set and adds
    none."""
    base, problem, launch_at, _ = POISON[name]
    M, O, B = CASES[name][:3]
    R = CASES[name][-1]
    assert mirror_chain(base)[2] >= 1e-9
    want, clean, got = [], [], []
    with np.errstate(invalid="ignore"):
        visited = mirror_chain(name, trace=want)[3]
    assert all(row[problem] is not None for row in visited[launch_at:launch_at + 2])
    device_chain(dev, base, per_thread, trace=clean)
    device_chain(dev, name, per_thread, trace=got)
    others = [b for b in range(B) if b != problem]
    for r in range(LAUNCHES):
        (w, wh), (c, ch), (g, gh) = want[r], clean[r], got[r]
        poisoned = np.zeros((B, M), dtype=bool)
        poisoned[problem] = r >= launch_at
        assert np.array_equal(np.isnan(w), poisoned), r               # what the mirror says
        assert np.array_equal(np.isnan(g), poisoned), r               # taken at launch_at, kept after
        assert np.array_equal(np.isinf(g), np.isinf(w)), r
        seen = np.isfinite(w)
        if seen.any():
            assert np.max(np.abs(clearance(g[seen], R) - clearance(w[seen], R))) <= 1e-13, r
        np.testing.assert_array_equal(gh, wh, err_msg=f"launch {r}")
        assert g[others].tobytes() == c[others].tobytes(), r
        assert np.array_equal(gh[others], ch[others]), r
        if r < launch_at:
            assert g.tobytes() == c.tobytes() and np.array_equal(gh, ch), r
    # the poisoned launch added nothing to its row of the counts; the clean chain did count there,
    # and the launches after it count as in the clean chain
    i = visited[launch_at][problem]
    assert got[-1][1][problem, i] == 7 < clean[-1][1][problem, i]
    later = [visited[r][problem] for r in range(launch_at + 1, LAUNCHES) if visited[r][problem] is not None]
    assert later and all(got[-1][1][problem, j] == clean[-1][1][problem, j] for j in later)


def test_stride_zero_shares_and_stride_one_separates(dev):
    """Two problems with the same state, step and obstacles: identical rows under stride 0,
    different ones under stride 1."""
    import torch
    M, O, nx = 257, 3, 4
    rng = np.random.default_rng(5)
    nominal = torch.from_numpy(np.tile(rng.uniform(-2, 2, size=(O, P, 2)), (2, 1, 1))).to(dev)
    x0 = torch.from_numpy(np.tile(rng.uniform(-2, 2, size=(1, nx)), (2, 1))).to(dev)
    state = torch.tensor([[0, 3], [0, 3]], dtype=torch.int64, device=dev)
    c_out = np.eye(2, nx)
    rows = {}
    for stride in (0, 1):
        min_d2 = torch.full((2, M), float("inf"), dtype=torch.float64, device=dev)
        hits = torch.zeros((2, 4), dtype=torch.int64, device=dev)
        mc.loop_clearance_step(x0, c_out, nominal, O, state, min_d2, hits, step_begin=0, log_rows=3,
                               noise_steps=P, robot_radius=0.5, obstacle_radius=0.5, seed=SEED,
                               noise_cov=LAPLACE_COV, eval_offset=2 ** 32 - 1,
                               problem_offset_stride=stride)
        assert bool(torch.isfinite(min_d2).all()) and not hits[:, :3].any()
        rows[stride] = min_d2
    assert torch.equal(rows[0][0], rows[0][1]) and not torch.equal(rows[1][0], rows[1][1])
    assert torch.equal(rows[0][0], rows[1][0])


def test_python_validation_errors(dev):
    import torch
    f64 = dict(dtype=torch.float64, device=dev)
    x0, nominal = torch.zeros((2, 4), **f64), torch.zeros((6, P, 2), **f64)
    state = torch.zeros((2, 2), dtype=torch.int64, device=dev)
    min_d2, hits = torch.zeros((2, 9), **f64), torch.zeros((2, 3), dtype=torch.int64, device=dev)
    kw = dict(step_begin=0, log_rows=2, robot_radius=0.5, obstacle_radius=0.5)
    c = np.eye(2, 4)
    mc.loop_clearance_step(x0, c, nominal, 3, state, min_d2, hits, **kw)
    bad = [dict(x0=x0.float()), dict(x0=x0[:, :3]), dict(x0=x0.cpu()), dict(c_out=np.eye(2, 3)),
           dict(nominal_path=nominal[:5]), dict(nominal_path=nominal.float()), dict(n_obstacles=2),
           dict(state=state[:1]), dict(state=state.int()), dict(min_d2=min_d2[:1]),
           dict(min_d2=min_d2[:, ::2]), dict(step_hits=hits[:, :2]), dict(step_hits=hits.int()),
           dict(step_hits=hits.cpu())]
    for change in bad:
        a = dict(x0=x0, c_out=c, nominal_path=nominal, n_obstacles=3, state=state, min_d2=min_d2,
                 step_hits=hits)
        a.update(change)
        with pytest.raises(ValueError):
            mc.loop_clearance_step(**a, **kw)
    for extra in (dict(noise="cauchy"), dict(realizations_per_thread=-1),
                  dict(realizations_per_thread=mc.LOOP_EVAL_MAX_PER_THREAD + 1), dict(noise_steps=-1)):
        with pytest.raises(ValueError):
            mc.loop_clearance_step(x0, c, nominal, 3, state, min_d2, hits, **kw, **extra)
