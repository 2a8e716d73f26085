"""Monte Carlo out-of-sample collision evaluation, CPU side (evaluation/monte_carlo.py,
evaluation/metrics.py, the host checks of drcvar_min_clearance_f64[_ex]).

The fixture tests/golden/monte_carlo/clearance_ref.npz was drawn by the reference's own
generate_laplace_realization / compute_distance_to_collision / safety_metrics with seed 42
(tests/golden/make_golden_mc.py).  The host backend must reproduce it bit for bit; the NumPy mirror
of the device kernel (tests/clearance_mirror.py) must draw the distributions the header promises.
None of these tests reaches a device.
"""
import ctypes
import os

import numpy as np
import pytest

import clearance_mirror as cm
from conftest import GOLDEN_DIR, load_golden
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.evaluation import metrics, monte_carlo as mc
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.environment import SafetyFilteringEnvironment


@pytest.fixture(scope="module")
def gold():
    return load_golden(os.path.join(GOLDEN_DIR, "monte_carlo", "clearance_ref.npz"))


def _env(gold):
    rr, ro = (float(v) for v in gold["radii"])
    return SafetyFilteringEnvironment(ROBOT_RADIUS=rr, OBSTACLE_RADIUS=ro, HORIZON=20, DT=0.2,
                                      ALPHA=0.2, DELTA=0.1, EPSILON=0.15)


def test_host_backend_reproduces_reference(gold):
    M = gold["realizations"].shape[0]
    np.random.seed(42)
    reals = mc.laplace_realizations_host(gold["nominal"], M, gold["noise_cov"])
    np.testing.assert_array_equal(np.array(reals), gold["realizations"])
    trajs = {"straight": gold["egos"][0], "shifted": gold["egos"][1]}
    res = mc.run_monte_carlo_simulation(_env(gold), trajs, gold["nominal"], M, backend="host", seed=42)
    keys = [str(k) for k in gold["metric_keys"]]
    for k, name in enumerate(trajs):
        np.testing.assert_array_equal(res[name]["step_distances"], gold["distances"][k])
        np.testing.assert_array_equal(res[name]["min_distances"], gold["distances"][k].min(axis=1))
        assert sorted(res[name]["metrics"]) == keys
        for j, key in enumerate(keys):
            want = gold["metrics"][k, j]
            assert abs(res[name]["metrics"][key] - want) <= 1e-15 * abs(want), key
        np.testing.assert_array_equal(res[name]["step_collision_rate"],
                                      (gold["distances"][k] < 0).mean(axis=0))
    # positions [T, 2] instead of states [T, 4]: the same numbers
    pos = mc.run_monte_carlo_simulation(_env(gold), {"p": gold["egos"][1][:, :2]}, gold["nominal"], M,
                                        backend="host", seed=42)
    np.testing.assert_array_equal(pos["p"]["step_distances"], gold["distances"][1])


def test_host_backend_step_rule_and_noise_kind(gold):
    """n_steps = min over the trajectories and the nominal paths (environment.py:119); the host
    procedure has no Gaussian form."""
    trajs = {"short": gold["egos"][0][:7], "long": gold["egos"][1]}
    res = mc.run_monte_carlo_simulation(_env(gold), trajs, gold["nominal"], 3, backend="host", seed=1)
    assert res["short"]["step_distances"].shape == res["long"]["step_distances"].shape == (3, 7)
    with pytest.raises(ValueError):
        mc.run_monte_carlo_simulation(_env(gold), trajs, gold["nominal"], 3, noise="gaussian", backend="host")
    with pytest.raises(ValueError):
        mc.run_monte_carlo_simulation(_env(gold), trajs, gold["nominal"], 3, backend="cpu")


def test_metrics_numpy(gold):
    keys = [str(k) for k in gold["metric_keys"]]
    for k in range(2):
        d = gold["distances"][k].min(axis=1)
        got = metrics.safety_metrics(d)
        assert sorted(got) == keys
        for j, key in enumerate(keys):
            assert abs(got[key] - gold["metrics"][k, j]) <= 1e-15 * abs(gold["metrics"][k, j])
    # hand cases
    d = np.array([0.5, 1.0, 2.0])
    assert metrics.collision_rate(d) == 0.0 and metrics.expectation_of_shortfall(d) == 0.0  # empty
    assert metrics.expectation_of_shortfall(d, threshold=1.5) == pytest.approx(-0.75)
    d = np.array([-1.0, -3.0])                                                           # all collide
    m = metrics.safety_metrics(d)
    assert m["collision_rate"] == 1.0 and m["expected_shortfall"] == -2.0 and m["median"] == -2.0
    assert m["q10"] == pytest.approx(-2.8) and m["q90"] == pytest.approx(-1.2)
    m = metrics.safety_metrics(np.array([0.25]))                                         # one element
    assert m["mean"] == m["min"] == m["max"] == m["median"] == m["q10"] == m["q90"] == 0.25
    assert m["std"] == 0.0 and m["collision_rate"] == 0.0 and m["expected_shortfall"] == 0.0


def test_metrics_torch_path_matches_numpy():
    """The torch path (sort + interpolation, run here on a CPU tensor) against np.percentile."""
    import torch
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 1000):
        d = rng.normal(0.1, 0.3, size=n)
        want, got = metrics.safety_metrics(d), metrics.safety_metrics(torch.from_numpy(d))
        assert list(got) == list(want)
        for key in want:
            assert isinstance(got[key], float)
            assert got[key] == pytest.approx(want[key], rel=1e-12, abs=1e-15), key
        assert metrics.collision_rate(torch.from_numpy(d)) == pytest.approx(metrics.collision_rate(d))
        assert metrics.expectation_of_shortfall(torch.from_numpy(d), 0.05) == \
            pytest.approx(metrics.expectation_of_shortfall(d, 0.05), rel=1e-12)
    assert metrics.expectation_of_shortfall(torch.tensor([1.0, 2.0], dtype=torch.float64)) == 0.0
    with pytest.raises(ValueError):
        metrics.safety_metrics(torch.zeros(3, dtype=torch.float32))


_CLEAN11 = np.array([0.3, -0.2, 1.5, 0.7, -1.1, 2.2, 0.05, 0.9, -0.4, 1.0, 0.6])


def _with(values, index, value):
    out = np.array(values, dtype=np.float64)
    out[index] = value
    return out


NON_FINITE_SAMPLES = {
    "clean": _CLEAN11,
    "one_nan": _with(_CLEAN11, 4, np.nan),
    "all_nan": np.full(11, np.nan),
    "one_inf": _with(_CLEAN11, 2, np.inf),
    "all_inf": np.full(11, np.inf),           # what an empty obstacle grid gives
    "upper_half_inf": _with(_CLEAN11, slice(5, None), np.inf),
    "all_inf_even": np.full(10, np.inf),
}


def _same(got, want):
    """The same NaN-ness, the same infinity, or within 1e-12 relative."""
    if np.isnan(want) or np.isinf(want):
        return bool(np.isnan(got)) if np.isnan(want) else got == want
    return abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("name", list(NON_FINITE_SAMPLES))
def test_metrics_torch_path_matches_numpy_on_non_finite_clearances(name):
    """The kernels propagate NaN (include/drcvar_sampling.h) and the statistics must not lose it:
    torch.sort puts NaN last, so the sorted order alone reads a finite minimum and finite quantiles
    out of a sample with a NaN, where NumPy's are NaN; and an all-+inf sample has the median +inf."""
    import torch
    import warnings
    d = NON_FINITE_SAMPLES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # NumPy's own inf - inf in std and lerp
        want = metrics.safety_metrics(d)
        want_rate = metrics.collision_rate(d)
        want_short = [metrics.expectation_of_shortfall(d, thr) for thr in (0, 0.65)]
    t = torch.from_numpy(d)
    got = metrics.safety_metrics(t)
    assert list(got) == list(want)
    for key in want:
        assert isinstance(got[key], float)
        assert _same(got[key], float(want[key])), (key, got[key], want[key])
    assert _same(metrics.collision_rate(t), float(want_rate))
    for thr, w in zip((0, 0.65), want_short):
        assert _same(metrics.expectation_of_shortfall(t, thr), float(w)), thr
    if name == "one_nan":
        assert all(np.isnan(got[k]) for k in ("mean", "min", "max", "std", "q10", "q25", "median", "q75", "q90"))
    if name == "all_inf":
        assert got["median"] == got["min"] == got["max"] == np.inf


def test_safety_statistics_keeps_a_nan_row_undefined():
    """closed_loop.safety_statistics, the arithmetic of LoopEvaluation's safety() on CPU tensors: a
    problem with a NaN clearance has collided = NaN (and NaN metrics), the clean problem next to it
    has exactly what it has alone."""
    import torch
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import closed_loop
    R = 0.5
    clean = np.array([0.04, 0.36, 1.0, 0.2499, 0.25, 9.0, np.inf, 0.0])       # d^2; R^2 = 0.25
    min_d2 = torch.from_numpy(np.stack([clean, _with(clean, 3, np.nan), clean[::-1].copy()]))
    hits = torch.tensor([[1, 2, 0], [0, 2, 0], [3, 0, 0]], dtype=torch.int64)
    res = closed_loop.safety_statistics(min_d2, hits, R)
    alone = closed_loop.safety_statistics(min_d2[:1], hits[:1], R)
    assert res["collided"].dtype == torch.float64 and tuple(res["collided"].shape) == (3,)
    assert res["collided"][0].item() == res["collided"][2].item() == 3 / 8 == alone["collided"][0].item()
    assert np.isnan(res["collided"][1].item())
    assert torch.equal(res["min_clearance"][0], alone["min_clearance"][0])
    assert torch.equal(res["min_clearance"][0], torch.sqrt(min_d2[0]) - R)
    assert torch.isnan(res["min_clearance"]).sum().item() == 1 and bool(torch.isnan(res["min_clearance"][1, 3]))
    assert all(_same(res["metrics"][0][k], v) for k, v in alone["metrics"][0].items())
    assert np.isnan(res["metrics"][1]["min"]) and np.isnan(res["metrics"][1]["median"])
    assert res["metrics"][0]["min"] == -R and res["metrics"][0]["max"] == np.inf
    assert torch.equal(res["step_hits"], hits)
    assert torch.equal(res["step_collision_rate"], hits.to(torch.float64) / 8)
    # the reference mode hands in clearances: negative = collided, NaN = undefined
    clr = torch.sqrt(min_d2) - R
    ref = closed_loop.safety_statistics(None, hits, R, clearance=clr)
    assert ref["collided"][0].item() == 3 / 8 and np.isnan(ref["collided"][1].item())
    assert ref["min_clearance"] is clr


def _clear(lib, ex=False, **kw):
    a = dict(ego=16, K=2, esk=20, est=2, nominal=16, O=3, T=5, nso=10, nst=2, kind=1, p0=0.07, p1=0.07,
             p2=0.0, R=0.6, m0=0, M=100, seed=1, stream=0, zero=1, out=16, osk=100, hits=None, splits=0)
    a.update(kw)
    args = [ctypes.c_void_p(a["ego"]), a["K"], a["esk"], a["est"], ctypes.c_void_p(a["nominal"]), a["O"],
            a["T"], a["nso"], a["nst"], a["kind"], a["p0"], a["p1"], a["p2"], a["R"], a["m0"], a["M"],
            a["seed"], a["stream"], a["zero"], ctypes.c_void_p(a["out"]), a["osk"], a["hits"]]
    if ex:
        return lib.drcvar_min_clearance_f64_ex(*args, a["splits"], None)
    return lib.drcvar_min_clearance_f64(*args, None)


@pytest.mark.parametrize("ex", [False, True])
def test_clearance_host_side_argument_validation(ex):
    """Every row of the limits table of include/drcvar_sampling.h, with dummy non-null pointers:
    each call returns from the host-side checks."""
    lib = _native.lib()
    call = lambda **kw: _clear(lib, ex, **kw)
    INV, UNS, OK = _native.ERR_INVALID_ARGUMENT, _native.ERR_UNSUPPORTED, _native.OK
    # outside the limits
    assert call(K=0) == UNS and call(K=9) == UNS
    assert call(O=2 ** 10 + 1, T=2 ** 10) == UNS and call(O=2 ** 21, T=1) == UNS
    assert call(m0=2 ** 40, M=1) == UNS and call(m0=0, M=2 ** 40 + 1) == UNS
    assert call(m0=2 ** 39, M=2 ** 39 + 1) == UNS
    # realisations per call: 256 per workgroup and at most 2^31 - 1 workgroups, so 2^39 itself is
    # over the grid's limit although m_begin + n_realizations <= 2^40 would allow it (the largest
    # accepted count, 2^39 - 256, would launch: not called here)
    assert call(m0=0, M=2 ** 39) == UNS and call(m0=0, M=2 ** 39 - 255) == UNS
    assert call(m0=0, M=2 ** 39, out=0) == INV        # an invalid call stays invalid
    # null pointer, negative size, NaN parameter, negative Laplace scale, negative radius
    assert call(ego=0) == INV and call(nominal=0) == INV and call(out=0) == INV
    for name in ("K", "O", "T", "M", "m0"):
        assert call(**{name: -1}) == INV, name
    for name in ("p0", "p1", "p2", "R"):
        assert call(**{name: float("nan")}) == INV, name
        assert call(kind=0, **{name: float("nan")}) == INV, name
    # the noise itself must be finite: an infinite scale or Cholesky entry, of either sign
    for name in ("p0", "p1", "p2"):
        for inf in (float("inf"), float("-inf")):
            assert call(**{name: inf}) == INV, name
            assert call(kind=0, **{name: inf}) == INV, name
            assert call(M=0, **{name: inf}) == INV, name
    assert call(p0=-0.1) == INV and call(p1=-0.1) == INV and call(R=-0.6) == INV
    assert call(kind=2) == INV and call(kind=-1) == INV
    assert call(kind=0, p0=-0.1, M=0) == OK           # a Cholesky factor may carry any sign
    if ex:
        assert call(splits=-1) == INV
    # nothing to do: OK with nothing launched
    assert call(M=0) == OK
    assert call(M=0, O=0) == OK and call(M=0, T=0) == OK
    assert call(M=0, ego=0, nominal=0, out=0) == OK
    assert call(M=0, m0=2 ** 40) == OK                # the accepted edge of the realisation range
    assert call(M=0, O=2 ** 10, T=2 ** 10) == OK      # the accepted edge of the unit grid
    assert call(M=0, K=8) == OK and call(M=0, K=1) == OK


def test_python_surface_rejects_cpu_inputs():
    import torch
    ego, nom = torch.zeros(1, 3, 2, dtype=torch.float64), torch.zeros(2, 3, 2, dtype=torch.float64)
    with pytest.raises(ValueError):
        mc.min_clearance_device(ego, nom, 4, robot_radius=0.3, obstacle_radius=0.3)


M_STAT = 200_000


@pytest.fixture(scope="module")
def mirror_noise():
    b = np.sqrt(0.01 / 2)
    lap = cm.noise("laplace", (b, 2 * b), 1, 2, M_STAT, seed=7, zero_first_step=False)
    gau = cm.noise("gaussian", (0.1, 0.0, 0.1), 1, 2, M_STAT, seed=7, zero_first_step=False)
    return b, lap.reshape(M_STAT, 2, 2), gau.reshape(M_STAT, 2, 2)


def test_mirror_zero_first_step_and_windows():
    b = 0.07
    a = cm.noise("laplace", (b, b), 2, 3, 50, seed=3, stream_offset=5)
    assert not a[:, :, 0].any() and a[:, :, 1:].all()
    w = cm.noise("laplace", (b, b), 2, 3, 20, seed=3, stream_offset=5, first_realization=10)
    np.testing.assert_array_equal(w, a[10:30])
    assert not np.array_equal(a, cm.noise("laplace", (b, b), 2, 3, 50, seed=3, stream_offset=6))


def test_mirror_distributions(mirror_noise):
    """The mirror's draws at M = 200 000, O = 1, T = 2 (both steps noisy): per-axis mean within
    5 standard errors; variance within 6 sqrt(5 / M) relative for the Laplace kind (fourth moment
    6 sigma^4: the sample variance has relative standard deviation sqrt(5 / M)) and 6 sqrt(2 / M)
    for the Gaussian; KS against the exact CDF with p > 1e-4; correlation between axes and between
    steps below 5 / sqrt(M)."""
    from scipy import stats
    b, lap, gau = mirror_noise
    M = M_STAT
    for x, dists, rel in ((lap, (stats.laplace(scale=b), stats.laplace(scale=2 * b)), 6 * np.sqrt(5.0 / M)),
                          (gau, (stats.norm(scale=0.1), stats.norm(scale=0.1)), 6 * np.sqrt(2.0 / M))):
        for axis, dist in enumerate(dists):
            for t in range(2):
                v = x[:, t, axis]
                sd = dist.std()
                assert abs(v.mean()) < 5 * sd / np.sqrt(M)
                assert abs(v.var() / sd ** 2 - 1) < rel
                assert stats.kstest(v, dist.cdf).pvalue > 1e-4
        flat = x.reshape(M, 4)
        c = np.corrcoef(flat.T)
        assert np.max(np.abs(c - np.eye(4))) < 5 / np.sqrt(M)
    # a Laplace draw is not normal (and the test above can tell): excess kurtosis 3
    assert abs(stats.kurtosis(lap[:, 1, 0]) - 3.0) < 0.5
    assert stats.kstest(lap[:, 1, 0], stats.norm(scale=np.sqrt(2) * b).cdf).pvalue < 1e-4


def test_mirror_clearance_definitions():
    """min_clearance and step_hits by the header's definitions on a hand case."""
    ego = np.array([[[0.0, 0.0], [1.0, 0.0]]])                   # K = 1, T = 2
    nominal = np.array([[[3.0, 4.0], [1.0, 2.0]], [[0.0, 1.0], [9.0, 9.0]]])
    nz = np.zeros((2, 2, 2, 2))
    nz[1, 0, 1] = [0.0, -1.5]                                    # realisation 1: obstacle 0 at (1, 0.5)
    clr, hits, margin = cm.min_clearance(ego, nominal, nz, 0.75)
    np.testing.assert_allclose(clr, [[0.25, -0.25]], atol=1e-15)
    np.testing.assert_array_equal(hits, [[0, 1]])
    assert margin == pytest.approx(0.75 ** 2 - 0.25)
