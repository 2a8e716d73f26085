"""GPU: halfspaces straight from the nominal paths (drcvar_sampled_halfspaces_f64,
csrc/drcvar_sampled.hip) on the grid of tests/sampled_reference.py (3 obstacles x 4 steps, step 0
noise-free).

* the draw (``samples_out``) equals the stored sampler's (``sample_units_device``) bit for bit;
* every record lies within the derived bounds of tests/halfspace_reference.py's long-double
  reference ON THAT DRAW (bounds that hold for any summation order, none loosened), at every plan's
  full size, one pair into its last row and an odd size, in the six alpha classes and for an
  isotropic and a general factor — tests/test_sampled_host.py shows on the CPU that a rank off by
  one would fail these comparisons;
* the tie and fallback cases, with the window mirror's classes counted per plan.  Which plan can
  reach which class: every plan reaches SETTLED and FAST; the 64 x 1 plan (N <= 128) cannot be
  CROWDED (a bucket holds at most N <= 128 samples), and its window — at least 12 standard errors
  of the sample quantile either side — is at N <= 128 wider than |z_alpha| in every alpha class, so
  a unit whose samples all sit at mu_d is inside it: neither BELOW nor ABOVE.  Every other plan
  reaches all five;
* unit windows, determinism, failure exits, graph replay and the Python surface.
"""
import functools

import numpy as np
import pytest
import torch

import halfspace_reference as hr
import sampled_reference as sr
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import obstacles as ob

pytestmark = pytest.mark.gpu
SEED, STREAM = 11, 3
U = sr.O * sr.T


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _inputs(device):
    nominal, ego, ego_u = sr.grid()
    return torch.from_numpy(nominal).to(device), torch.from_numpy(ego).to(device), ego_u


def _params(alpha, epsilon=hr.EPSILON):
    return RiskParams(hr.RR, hr.RO, alpha, hr.DELTA, epsilon)


def _run(dev, n, chol, alpha, seed=SEED, stream_offset=STREAM, keep=False, epsilon=hr.EPSILON,
         nominal=None, **kw):
    """One sampled launch on the grid into a NaN-filled `out`: (records [U or count, 8] numpy,
    status numpy, samples_out tensor or None)."""
    nom, ego, _ = _inputs(dev)
    nom = nom if nominal is None else nominal
    count = kw.get("unit_count", None)
    rows = U - kw.get("unit_begin", 0) if count is None else count
    whole = count is None and kw.get("unit_begin", 0) == 0
    out = torch.full((sr.O, sr.T, 8) if whole else (rows, 8), float("nan"), dtype=torch.float64, device=dev)
    status = torch.full((rows,), -1, dtype=torch.int32, device=dev)
    samples = torch.full((rows, n, 2), float("nan"), dtype=torch.float64, device=dev) if keep else None
    engine.sampled_halfspaces(nom, ego, n, _params(alpha, epsilon), chol=chol, seed=seed, stream_offset=stream_offset,
                              out=out, status=status, samples_out=samples, **kw)
    return out.reshape(-1, 8).cpu().numpy(), status.cpu().numpy(), samples


@functools.lru_cache(maxsize=64)
def _stored(device, n, chol, zero_first=True, seed=SEED, stream_offset=STREAM):
    """The stored sampler's draw of the grid, flat [U, N, 2] (device tensor) and as numpy."""
    nom, _, _ = _inputs(device)
    s = torch.empty((U, n, 2), dtype=torch.float64, device=device)
    _native.check(_native.lib().drcvar_sample_units_f64(
        nom.data_ptr(), sr.O, sr.T, nom.stride(0), nom.stride(1), 0, U, n, *chol, seed, stream_offset,
        1 if zero_first else 0, s.data_ptr(), s.stride(0), s.stride(1),
        torch.cuda.current_stream(device).cuda_stream))
    return s, s.cpu().numpy()


def _compare(rec, ref, what):
    """Every column of every record against the reference, each at its own bound."""
    tag = f"{what}: "
    for c, b in ((0, ref.bound_hm), (1, ref.bound_hm), (2, ref.bound_gm), (3, ref.bound_h), (4, ref.bound_h),
                 (5, ref.bound), (6, ref.bound), (7, ref.bound)):
        err = np.abs(rec[:, c] - ref.rec[:, c])
        assert np.all(err <= b), tag + f"column {c}: err {err.max():.3e} at unit {int(np.argmax(err - b))}, " \
                                       f"bound {b[int(np.argmax(err - b))]:.3e}"


# ---------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,chol,zero_first,seed,stream", [
    (1000, sr.ISO, True, SEED, STREAM), (1000, sr.GENERAL, True, SEED, STREAM),
    (1001, sr.ISO, True, SEED, STREAM), (1001, sr.GENERAL, False, SEED, STREAM),
    (1, sr.ISO, False, SEED, STREAM), (1, sr.GENERAL, True, SEED, 0),
    (2, sr.ISO, False, SEED, 0), (129, sr.ISO, False, SEED, STREAM),
    (1000, sr.ISO, True, (1 << 40) + 12345, STREAM), (5001, sr.GENERAL, True, SEED, (1 << 33) + 7),
    (16384, sr.ISO, True, SEED, STREAM), (16383, sr.GENERAL, False, (1 << 63) + 5, STREAM),
    (8193, sr.ISO, True, SEED, STREAM), (3000, sr.GENERAL, True, SEED, STREAM)])
def test_draw_is_the_stored_samplers_bit_for_bit(dev, n, chol, zero_first, seed, stream):
    rec, st, got = _run(dev, n, chol, 0.2, seed=seed, stream_offset=stream, keep=True,
                        zero_first_step=zero_first)
    want, _ = _stored(dev, n, chol, zero_first, seed, stream)
    assert torch.equal(got, want)
    rec2, st2, _ = _run(dev, n, chol, 0.2, seed=seed, stream_offset=stream, zero_first_step=zero_first)
    assert rec.tobytes() == rec2.tobytes() and np.array_equal(st, st2)   # samples_out changes no bit
    assert not np.isnan(rec).any() and np.all(st == _native.UNIT_OK)


def test_samples_out_layouts(dev):
    """[O, T, N, 2] for the whole grid, and a strided [units, N, 2] view: the same values, nothing
    written between the units."""
    nom, ego, _ = _inputs(dev)
    want, _ = _stored(dev, 300, sr.GENERAL)
    s4 = torch.full((sr.O, sr.T, 300, 2), float("nan"), dtype=torch.float64, device=dev)
    engine.sampled_halfspaces(nom, ego, 300, _params(0.2), chol=sr.GENERAL, seed=SEED,
                              stream_offset=STREAM, samples_out=s4)
    assert torch.equal(s4.reshape(U, 300, 2), want)
    big = torch.full((2 * U, 300, 3), -7.0, dtype=torch.float64, device=dev)
    engine.sampled_halfspaces(nom, ego, 300, _params(0.2), chol=sr.GENERAL, seed=SEED,
                              stream_offset=STREAM, samples_out=big[::2, :, :2], unit_count=U)
    assert torch.equal(big[::2, :, :2], want)
    assert bool((big[1::2] == -7.0).all()) and bool((big[:, :, 2] == -7.0).all())


# ---------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", sr.PLANS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_records_within_the_reference_bounds(dev, plan):
    for n in sr.sizes_of(plan):
        assert _native.sampled_launch_plan(n) == plan[:2]
        for chol in sr.factors_of(n):
            _, s = _stored(dev, n, chol)
            _, _, ego_u = _inputs(dev)
            for a0 in hr.A0:
                alpha, m = hr.alpha_of(n, a0)
                ref = hr.reference(s, ego=ego_u, alpha=alpha)
                rec, st, _ = _run(dev, n, chol, alpha)
                assert np.all(st == _native.UNIT_OK)
                _compare(rec, ref, f"N={n} chol={chol} a0={a0}")


TIE_FACTORS = {"zero": (0.0, 0.0, 0.0), "sub_ulp": (1e-20, 0.0, 1e-20), "few_values": (3e-15, 0.0, 3e-15),
               "few_values_general": (3e-15, 1e-15, 2e-15), "x_only": (0.1, 0.0, 0.0)}


@pytest.mark.parametrize("plan", sr.PLANS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_fallback_and_ties(dev, plan):
    """The same comparison where the window cannot finish the selection: a zero factor (every unit
    all-equal, no window), noise below one ulp of the position (sd_d > 0, all samples one point),
    l = 3e-15 (a few dozen distinct values, crowded buckets), noise along x only — with
    zero_first_step off and on.  Together with the Gaussian units the mirror's classes are counted:
    the plan reaches every class it can (module docstring)."""
    _, _, ego_u = _inputs(dev)
    seen = {}
    n = sr.capacity(plan)
    for name, chol in list(TIE_FACTORS.items()) + [("gauss", sr.factors_of(n)[0])]:
        for zero_first in ((True, False) if name == "sub_ulp" else (True,)):
            _, s = _stored(dev, n, chol, zero_first)
            if name in ("zero", "sub_ulp"):
                assert np.all(s == s[:, :1])            # every sample of a unit the same point
            for a0 in hr.A0:
                alpha, _ = hr.alpha_of(n, a0)
                ref = hr.reference(s, ego=ego_u, alpha=alpha)
                rec, st, _ = _run(dev, n, chol, alpha, zero_first_step=zero_first)
                assert np.all(st == _native.UNIT_OK)
                _compare(rec, ref, f"{name} N={n} zf={zero_first} a0={a0}")
                for c in sr.classify_units(s, ref, chol, alpha, plan[2], zero_first):
                    seen[c] = seen.get(c, 0) + 1
    print(f"plan {plan}: classes {seen}")
    want = set(sr.CLASSES) if plan != sr.PLANS[0] else {sr.SETTLED, sr.FAST}
    assert want <= set(seen), (plan, seen)
    assert seen.get(sr.NOWINDOW, 0) > 0


# ---------------------------------------------------------------------------------------------
# windows, determinism
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,chol", [(1000, sr.ISO), (129, sr.GENERAL), (5001, sr.ISO)])
def test_unit_windows_and_determinism(dev, n, chol):
    whole, st, _ = _run(dev, n, chol, 0.2)
    again, st2, _ = _run(dev, n, chol, 0.2)
    assert whole.tobytes() == again.tobytes() and np.array_equal(st, st2)
    # windows that start mid-obstacle, span an obstacle boundary, hold one unit, are empty
    for begin, count in ((1, 2), (2, 5), (3, 1), (4, 8), (0, U), (5, 7), (U, 0), (6, 0)):
        part, pst, psamp = _run(dev, n, chol, 0.2, unit_begin=begin, unit_count=count, keep=True)
        assert part.shape == (count, 8)
        assert part.tobytes() == whole[begin:begin + count].tobytes(), (begin, count)
        assert np.array_equal(pst, st[begin:begin + count])
        assert torch.equal(psamp, _stored(dev, n, chol)[0][begin:begin + count])
    # another seed or stream: every noisy unit's record changes, the noise-free ones do not
    noisy = ~sr.noise_free_units()
    for kw in (dict(seed=SEED + 1), dict(stream_offset=STREAM + 1)):
        other, _, _ = _run(dev, n, chol, 0.2, **kw)
        changed = np.any(other[:, 3:] != whole[:, 3:], axis=1)
        assert np.all(changed[noisy]) and not np.any(changed[~noisy])
        assert np.all(other[noisy, 5] != whole[noisy, 5])


# ---------------------------------------------------------------------------------------------
# failure exits
# ---------------------------------------------------------------------------------------------
def _stored_records(dev, s, alpha, epsilon=hr.EPSILON):
    """The stored path on the same draw: (records, status)."""
    _, ego, _ = _inputs(dev)
    st = torch.full((U,), -1, dtype=torch.int32, device=dev)
    rec = engine.safe_halfspaces(s.reshape(sr.O, sr.T, -1, 2), ego, _params(alpha, epsilon), status=st)
    return rec.reshape(U, 8).cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("n", [100, 1000, 5001])
def test_failure_exits(dev, n):
    nom, _, ego_u = _inputs(dev)
    good, _, _ = _run(dev, n, sr.ISO, 0.2)
    # one NaN nominal position: that unit's sentinels and UNIT_NONFINITE, every other unit unchanged
    for bad_u, coord in ((5, 0), (4, 1)):
        nan_nom = nom.clone()
        nan_nom.reshape(U, 2)[bad_u, coord] = float("nan")
        rec, st, _ = _run(dev, n, sr.ISO, 0.2, nominal=nan_nom)
        others = np.arange(U) != bad_u
        assert rec[others].tobytes() == good[others].tobytes()
        assert st[bad_u] == _native.UNIT_NONFINITE and np.all(st[others] == _native.UNIT_OK)
        assert rec[bad_u, 5] == hr.SENTINEL and rec[bad_u, 6] == hr.SENTINEL
        s = torch.empty((U, n, 2), dtype=torch.float64, device=dev)
        ob.sample_units_device(nan_nom, n, 0, U, seed=SEED, stream_offset=STREAM, out=s)
        srec, sst = _stored_records(dev, s, 0.2)
        assert np.array_equal(st, sst)
        assert np.array_equal(np.isnan(rec), np.isnan(srec))
        assert np.array_equal(rec[bad_u, 5:7], srec[bad_u, 5:7])
    # alpha > 1 and epsilon < 0: the status bits and sentinels of the stored path on the same draw
    s, s_np = _stored(dev, n, sr.ISO)
    for alpha, eps, want in ((1.5, hr.EPSILON, _native.UNIT_UNBOUNDED),
                             (0.2, -0.05, _native.UNIT_DR_UNBOUNDED),
                             (1.5, -0.05, _native.UNIT_UNBOUNDED | _native.UNIT_DR_UNBOUNDED)):
        rec, st, _ = _run(dev, n, sr.ISO, alpha, epsilon=eps)
        srec, sst = _stored_records(dev, s, alpha, eps)
        assert np.all(st == want) and np.array_equal(st, sst)
        ref = hr.reference(s_np, ego=ego_u, alpha=alpha, epsilon=eps)
        _compare(rec, ref, f"alpha={alpha} eps={eps}")
        _compare(srec, ref, f"stored alpha={alpha} eps={eps}")
        if want & _native.UNIT_UNBOUNDED:
            assert np.all(rec[:, 5] == hr.SENTINEL) and np.all(rec[:, 6] == hr.SENTINEL)
        else:
            assert np.all(rec[:, 6] == hr.SENTINEL) and np.all(rec[:, 5] != hr.SENTINEL)


# ---------------------------------------------------------------------------------------------
# graph, Python surface
# ---------------------------------------------------------------------------------------------
def test_prepared_launch_in_a_graph(dev):
    nom, ego, _ = _inputs(dev)
    eager, st, _ = _run(dev, 1000, sr.ISO, 0.2)
    out = torch.full((sr.O, sr.T, 8), float("nan"), dtype=torch.float64, device=dev)
    status = torch.full((U,), -1, dtype=torch.int32, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream(dev)):   # one stream, no branches
        launch, _ = engine.prepare_sampled_halfspaces(nom, ego, 1000, _params(0.2), chol=sr.ISO, seed=SEED,
                                                      stream_offset=STREAM, out=out, status=status,
                                                      stream=torch.cuda.current_stream(dev))
        launch()
    for _ in range(2):
        out.fill_(float("nan"))
        status.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert out.reshape(U, 8).cpu().numpy().tobytes() == eager.tobytes()
        assert np.array_equal(status.cpu().numpy(), st)


def test_python_surface_against_the_two_launch_path(dev):
    nom, ego, ego_u = _inputs(dev)
    cov = np.array([[0.04, 0.012], [0.012, 0.02]])
    for n in (200, 1000):
        s = ob.sample_trajectories_device(nom, n, cov, seed=5, stream_offset=2)
        two = engine.safe_halfspaces(s, ego, _params(0.2)).reshape(U, 8).cpu().numpy()
        one = engine.sampled_halfspaces(nom, ego, n, _params(0.2), noise_cov=cov, seed=5, stream_offset=2)
        assert one.shape == (sr.O, sr.T, 8)
        ref = hr.reference(s.reshape(U, n, 2).cpu().numpy(), ego=ego_u, alpha=0.2)
        _compare(one.reshape(U, 8).cpu().numpy(), ref, f"sampled N={n}")
        _compare(two, ref, f"two-launch N={n}")
    # input checks, before any launch
    with pytest.raises(ValueError):
        engine.sampled_halfspaces(nom, ego, _native.MAX_SAMPLES + 1)
    with pytest.raises(ValueError):
        engine.sampled_halfspaces(nom, ego, 0)
    with pytest.raises(ValueError):
        engine.sampled_halfspaces(nom, ego[:3], 100)
    with pytest.raises(ValueError):
        engine.sampled_halfspaces(nom, ego, 100, unit_begin=5, unit_count=8)
    with pytest.raises(ValueError):
        engine.sampled_halfspaces(nom, ego, 100, out=torch.empty((U, 8), dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        engine.sampled_halfspaces(nom, ego, 100, samples_out=torch.empty((U, 99, 2), dtype=torch.float64, device=dev))
    with pytest.raises(np.linalg.LinAlgError):
        engine.sampled_halfspaces(nom, ego, 100, noise_cov=np.zeros((2, 2)))
    assert engine.sampled_halfspaces(nom, ego, 100, chol=(0.0, 0.0, 0.0)).shape == (sr.O, sr.T, 8)
    assert engine.sampled_halfspaces(nom, ego, 100, unit_begin=3, unit_count=4).shape == (4, 8)


def test_environment_feeds_the_mpc_filter(dev):
    """compute_halfspace_batch_sampled on multi_obstacle's nominal paths: the record feeds the
    device MPC filter, which returns an optimal solve."""
    import os

    from conftest import GOLDEN_DIR
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.config.scenarios import get_scenario_config
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core.mpc_filter import MPCSafetyFilter
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.environment import (
        SafetyFilteringEnvironment)
    m = np.load(os.path.join(GOLDEN_DIR, "mpc_multi_obstacle_h30.npz"), allow_pickle=False)
    H = int(m["horizon"])
    data = ob.generate_obstacle_scenarios_device(get_scenario_config("multi_obstacle"), 30.0, 0.2, 8,
                                                 seed=5, device=dev)
    env = SafetyFilteringEnvironment(ROBOT_RADIUS=0.3, OBSTACLE_RADIUS=0.3, HORIZON=H, DT=0.2,
                                     ALPHA=0.2, DELTA=0.1, EPSILON=0.15)
    batch = env.compute_halfspace_batch_sampled(data["nominal_trajectories"], m["x_ref"], 1000,
                                                ob.NOISE_COV, seed=5)
    n_obs = len(data["nominal_trajectories"])
    assert tuple(batch.record.shape) == (n_obs, H, 8) and not bool(torch.isnan(batch.record).any())
    # the same record as the stored path on the same draw, to rounding
    nom_d = torch.as_tensor(np.stack(data["nominal_trajectories"])).to(dev)[:, :H]
    s = ob.sample_trajectories_device(nom_d, 1000, ob.NOISE_COV, seed=5)
    ego_d = torch.as_tensor(np.ascontiguousarray(np.asarray(m["x_ref"])[:H] @ env.C.T)).to(dev)
    two = engine.safe_halfspaces(s, ego_d, env.params)
    assert float((two - batch.record).abs().max()) < 1e-9
    f = MPCSafetyFilter(m["A"], m["B"], m["C"], m["Q"], m["R"], H, 0.2)
    x, u, info = f.filter_trajectory(m["x0"], m["x_ref"], m["u_ref"], batch, tuple(m["u_bounds"]),
                                     tuple(m["p_bounds"]), metric="dr_cvar")
    assert info["status"] == "optimal", info
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(x))
