"""The HIP safety-filter QP (csrc/drcvar_mpc.hip) with boxes that bind: the input box alone, the
position box alone and both, every bound its own number, on every launch form (512 threads, the
128- and 256-thread many-problem forms, clusters with their rows in LDS and in global memory),
every input width and state template — the cases of tests/mpc_bound_cases.py, whose oracle-side
conditions (every side of every bounded component active somewhere in the case) are held by
tests/test_mpc_bounds_host.py.  All problems of a case go in one launch.

Per case: status and polish; inputs and states against the KKT-certified oracle; and from the
answer alone, for every problem — x[0] bitwise x0, x[1:] the extended-precision rollout of the
returned u, every u and C x inside its own component's bounds, the same (step, component, side)
at a bound as the oracle's optimum, and the info record's objective and largest slack recomputed
from the returned trajectory.

Polished shares the device reached (MI355X): 16 / 16 in every few case, 8 / 8 in every cluster
case on both launches, 144 / 144 in every many case; the largest |u - u_oracle| per group was
few 5.7e-7 (four inputs, input box alone), many 5.5e-8, cluster 1.1e-8 (docs/lab_notebook.md §5).
Before the polish required its equalities closed (csrc/drcvar_mpc.hip, kPolishLateTol), problem 3
of (double, 33, 3, "p") came back POLISHED 2.2e-6 from the oracle, in the few and the many form.

Two more: strided x0 / x_ref / u_fallback views in NaN-filled storage give the dense launch's bits,
and a batch that mixes a solved problem with two that take the fallback exit.
"""
import numpy as np
import pytest

import mpc_bound_cases as bc
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native
from oracle import mpc_qp
from test_mpc import MPC_TOL, _oracle
from test_mpc_cluster import _solve

OK_STATUS = (_native.MPC_STATUS_OPTIMAL, _native.MPC_STATUS_OPTIMAL_INACCURATE)
UNPOLISHED_TOL = 1e-5
# unpolished problems allowed per launch: 1 of 16, 1 of 8, 3 % of a many-problem launch
UNPOLISHED_CAP = {"few": lambda n: 1, "cluster": lambda n: 1, "many": lambda n: int(0.03 * n)}


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _rollout_error(prs, x, u):
    """max over steps and states of |x[b, 1:] - rollout in np.longdouble of u[b] from x0[b]|, [B]."""
    A = prs[0]["A"].astype(np.longdouble)
    Bm = prs[0]["B"].astype(np.longdouble)
    xl = np.stack([p["x0"] for p in prs]).astype(np.longdouble)
    ul = u.astype(np.longdouble)
    err = np.zeros(len(prs))
    for t in range(u.shape[1]):
        xl = xl @ A.T + ul[:, t] @ Bm.T
        err = np.maximum(err, np.abs(x[:, t + 1].astype(np.longdouble) - xl).max(axis=1).astype(np.float64))
    return err


def _check_answers(case, prs, x, u, info, label):
    """Every check of one launch's answers; returns (polished, largest |u - u_oracle|)."""
    group, dyn, H, O, form, n = case
    nx, nu = prs[0]["A"].shape[0], prs[0]["B"].shape[1]
    C = prs[0]["C"]
    assert x.shape == (n, H + 1, nx) and u.shape == (n, H, nu)
    status = info[:, _native.MPC_INFO_STATUS]
    assert np.all(np.isin(status, OK_STATUS)), (label, status)
    assert np.all(info[:, _native.MPC_INFO_USED_FALLBACK] == 0), label
    polished = info[:, _native.MPC_INFO_POLISHED] == 1
    print(f"{label}: polished {int(polished.sum())} / {n}, unpolished {np.flatnonzero(~polished).tolist()}")
    assert int((~polished).sum()) <= UNPOLISHED_CAP[group](n), (label, np.flatnonzero(~polished))

    # from the answer alone, every problem
    x0 = np.stack([p["x0"] for p in prs])
    np.testing.assert_array_equal(x[:, 0], x0, err_msg=label)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(u)), label
    err = _rollout_error(prs, x, u)
    roll_tol = 64 * (H * nu + nx) * 2.0 ** -53 * np.maximum(1.0, np.abs(x).max(axis=(1, 2)))
    print(f"{label}: rollout error {err.max():.2e}, smallest bound {roll_tol.min():.2e}")
    assert np.all(err <= roll_tol), (label, np.flatnonzero(err > roll_tol), err.max())
    pos = x[:, 1:] @ C.T                                       # [B, H, 2]
    if "u" in form:
        lo, hi = prs[0]["ub"]
        assert np.all(u >= lo - MPC_TOL) and np.all(u <= hi + MPC_TOL), \
            (label, (lo - u).max(axis=(0, 1)), (u - hi).max(axis=(0, 1)))
    if "p" in form:
        lo, hi = prs[0]["pb"]
        assert np.all(pos >= lo - MPC_TOL) and np.all(pos <= hi + MPC_TOL), \
            (label, (lo - pos).max(axis=(0, 1)), (pos - hi).max(axis=(0, 1)))
    hs = np.stack([p["hs"] for p in prs])                      # [B, O, H, 3]
    s_dev = np.maximum(0.0, np.einsum("botc,btc->bot", hs[..., :2], pos) + hs[..., 2])
    for b in np.flatnonzero(polished):
        obj = mpc_qp.objective(prs[b]["Q"], prs[b]["R"], x[b], u[b], prs[b]["x_ref"], s_dev[b])
        assert abs(info[b, _native.MPC_INFO_OBJECTIVE] - obj) <= 1e-10 * max(1.0, abs(obj)), \
            (label, b, info[b, _native.MPC_INFO_OBJECTIVE], obj)
        assert abs(info[b, _native.MPC_INFO_MAX_SLACK] - s_dev[b].max(initial=0.0)) <= 1e-10, (label, b)

    # against the oracle (which the active sets need too)
    worst = 0.0
    for b in bc.oracle_subset(case):
        xo, uo, io = bc.oracle(case, b)
        assert io["status"] == "optimal" and max(io["kkt"].values()) < 1e-8, (label, b)
        tol = MPC_TOL if polished[b] else UNPOLISHED_TOL
        worst = max(worst, float(np.abs(u[b] - uo).max()))
        np.testing.assert_allclose(u[b], uo, rtol=0, atol=tol, err_msg=f"{label} problem {b}")
        np.testing.assert_allclose(x[b], xo, rtol=0, atol=tol, err_msg=f"{label} problem {b}")
        if polished[b]:
            got = bc.active_sides(prs[b], x[b], u[b], MPC_TOL)
            want = bc.active_sides(prs[b], xo, uo, bc.ACTIVE_TOL)
            assert got == want, (label, b, sorted(got - want), sorted(want - got))
    print(f"{label}: largest |u - u_oracle| {worst:.2e} over {len(bc.oracle_subset(case))} problems")
    return polished, worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_gpu_active_bounds_match_oracle(case, dev):
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core import mpc_filter as mf
    group, dyn, H, O, form, n = case
    prs = bc.problems(case)
    assert len(prs) == n
    x, u, info, groups = _solve(prs, dev)
    if group == "cluster":
        assert groups > 1
    else:
        assert groups == 1
        assert n > 128 if group == "many" else n <= 128
    pol, _ = _check_answers(case, prs, x, u, info, bc.case_id(case))
    if group == "cluster":  # the same problems on one workgroup each
        x1, u1, info1, g1 = _solve(prs, dev, mf.make_options(cluster_size=1))
        assert g1 == 1
        pol1, _ = _check_answers(case, prs, x1, u1, info1, bc.case_id(case) + " one workgroup")
        both = pol & pol1
        np.testing.assert_allclose(u[both], u1[both], rtol=0, atol=MPC_TOL)
        np.testing.assert_allclose(x[both], x1[both], rtol=0, atol=MPC_TOL)


@pytest.mark.gpu
def test_gpu_strided_inputs_give_the_dense_bits(dev):
    """x0, x_ref and u_fallback as views with a contiguous last dimension inside larger storage
    (the x0_sp, xr_sp, xr_st, uf_sp, uf_st of drcvar_mpc_filter_f64), everything outside the views
    NaN: x, u and info are the dense launch's bit for bit."""
    import torch
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core import mpc_filter as mf
    case = ("few", "double", 12, 3, "up", bc.N_FEW)
    prs = bc.problems(case)
    p0 = prs[0]
    H, nx, nu, n = p0["H"], 4, 2, len(prs)
    xd, ud, infod, _ = _solve(prs, dev)
    big_x0 = np.full((n, nx + 3), np.nan)
    big_xr = np.full((n, H + 4, nx + 2), np.nan)
    big_uf = np.full((n, H + 3, nu + 2), np.nan)
    big_x0[:, 1:1 + nx] = np.stack([p["x0"] for p in prs])
    big_xr[:, 2:2 + H + 1, :nx] = np.stack([p["x_ref"] for p in prs])
    big_uf[:, 2:2 + H, :nu] = np.stack([p["u_ref"] for p in prs])
    T_ = lambda a: torch.as_tensor(a).to(dev)
    x0 = T_(big_x0)[:, 1:1 + nx]
    xr = T_(big_xr)[:, 2:2 + H + 1, :nx]
    uf = T_(big_uf)[:, 2:2 + H, :nu]
    assert not x0.is_contiguous() and not xr.is_contiguous() and not uf.is_contiguous()
    assert (x0.stride(0), xr.stride(0), xr.stride(1), uf.stride(0), uf.stride(1)) == \
        (nx + 3, (H + 4) * (nx + 2), nx + 2, (H + 3) * (nu + 2), nu + 2)
    model = mf.MPCModel(p0["A"], p0["B"], p0["C"], p0["Q"], p0["R"], H, p0["ub"], p0["pb"], device=dev)
    hs = T_(np.stack([p["hs"] for p in prs]))
    x, u, info = mf.filter_batch(model, hs[..., 0:2], hs[..., 2], x0, xr, uf)
    np.testing.assert_array_equal(x.cpu().numpy(), xd)
    np.testing.assert_array_equal(u.cpu().numpy(), ud)
    np.testing.assert_array_equal(info.cpu().numpy(), infod)
    assert np.all(np.isfinite(xd)) and np.all(np.isfinite(ud))


@pytest.mark.gpu
def test_gpu_batch_mixes_solved_and_fallback_problems(dev):
    """One launch of three problems on tests/test_mpc.py's infeasible model: 0 and 2 cannot reach
    the position box and return their own rows of a strided u_fallback rolled out, 1 starts inside
    the box and is solved."""
    import torch
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core import mpc_filter as mf
    prs = bc.mixed_batch()
    p0 = prs[0]
    H, nx, nu = p0["H"], 4, 2
    xo, uo, io = _oracle(prs[1])
    assert io["status"] == "optimal" and max(io["kkt"].values()) < 1e-8
    big_uf = np.full((3, H + 3, nu + 2), np.nan)
    big_uf[:, 2:2 + H, :nu] = np.stack([p["u_ref"] for p in prs])
    T_ = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    uf = T_(big_uf)[:, 2:2 + H, :nu]
    model = mf.MPCModel(p0["A"], p0["B"], p0["C"], p0["Q"], p0["R"], H, p0["ub"], p0["pb"], device=dev)
    hs = T_(np.stack([p["hs"] for p in prs]))
    x, u, info = mf.filter_batch(model, hs[..., 0:2], hs[..., 2], T_(np.stack([p["x0"] for p in prs])),
                                 T_(np.stack([p["x_ref"] for p in prs])), uf)
    x, u, info = x.cpu().numpy(), u.cpu().numpy(), info.cpu().numpy()
    assert int(info[1, _native.MPC_INFO_STATUS]) in OK_STATUS, info[1]
    assert info[1, _native.MPC_INFO_USED_FALLBACK] == 0
    np.testing.assert_allclose(u[1], uo, rtol=0, atol=MPC_TOL)
    np.testing.assert_allclose(x[1], xo, rtol=0, atol=MPC_TOL)
    for b in (0, 2):
        assert info[b, _native.MPC_INFO_USED_FALLBACK] == 1, info[b]
        assert int(info[b, _native.MPC_INFO_STATUS]) not in OK_STATUS, info[b]
        np.testing.assert_array_equal(u[b], prs[b]["u_ref"])
        np.testing.assert_allclose(x[b], mpc_qp.rollout(p0["A"], p0["B"], prs[b]["x0"], prs[b]["u_ref"]),
                                   rtol=0, atol=1e-12)
    assert not np.array_equal(u[0], u[2])
