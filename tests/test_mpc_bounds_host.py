"""The conditions that keep tests/test_mpc_bounds_gpu.py from being vacuous, checked with the
oracle alone (oracle/mpc_qp.py) on the cases of tests/mpc_bound_cases.py: per case and form every
problem is KKT-certified, every side of every bounded component is active in at least one
problem's optimum, some halfspace slack is positive and some row is active at zero slack, and all
bound values of a model differ in absolute value.  A many-problem case is looked at through its
first 16 problems (the generator cycles the box's corners with the problem's number).
"""
import numpy as np
import pytest

import mpc_bound_cases as bc


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_oracle_certifies_and_every_bound_side_is_active(case):
    group, dyn, H, O, form, n = case
    n = min(n, bc.HOST_PROBLEMS)
    prs = bc.problems(case)[:n]
    nu = prs[0]["B"].shape[1]
    positive_slack = zero_slack_active = 0
    for k, pr in enumerate(prs):
        assert (pr["ub"] is not None) == ("u" in form) and (pr["pb"] is not None) == ("p" in form)
        x, u, io = bc.oracle(case, k)
        assert io["status"] == "optimal", (k, io["status"])
        assert max(io["kkt"].values()) < 1e-8, (k, io["kkt"])
        r = bc.halfspace_residuals(pr, x)                      # [O, H]; the slacks are step-major
        s = io["slacks"].reshape(H, O).T
        np.testing.assert_allclose(np.maximum(r, 0.0), s, atol=1e-8)
        positive_slack += bool((s > 1e-6).any())
        zero_slack_active += bool(((np.abs(r) < bc.ACTIVE_TOL) & (s < bc.ACTIVE_TOL)).any())
    counts = bc.side_counts(case, n)
    print(bc.case_id(case), {f"{kind}_{'min' if side == 0 else 'max'}[{i}]": c
                             for (kind, i, side), c in counts.items()})
    assert len(counts) == (2 * nu if "u" in form else 0) + (4 if "p" in form else 0)
    idle = [key for key, c in counts.items() if c == 0]
    assert not idle, f"sides never active: {idle}"
    assert positive_slack >= 1 and zero_slack_active >= 1, (positive_slack, zero_slack_active)


@pytest.mark.parametrize("case", [c for c in bc.CASES if c[4] == "u"], ids=bc.case_id)
def test_bound_values_pairwise_distinct_in_absolute_value(case):
    pr = bc.problems(case)[0]
    nu = pr["B"].shape[1]
    v = np.sort(np.abs(bc.bound_values(pr)))
    assert v.size == 2 * nu + 4
    assert np.all(np.diff(v) > 1e-3), v
    np.testing.assert_array_equal(np.concatenate(pr["ub"]), bc.bound_values(pr)[:2 * nu])
    up = bc.problems(case[:4] + ("up",) + case[5:])[0] if case[1] != "generic1" else None
    if up is not None:                                         # the forms select among one set
        np.testing.assert_array_equal(np.concatenate(up["ub"] + up["pb"]), bc.bound_values(pr))


def test_generator_aims_each_problem_at_its_corner():
    """Problem k starts inside the position box within 0.8 of corner k mod 4, its reference ends
    outside the box beyond that corner on both axes, and x0 carries a velocity."""
    case = ("few", "double", 12, 3, "up", bc.N_FEW)
    for k, pr in enumerate(bc.problems(case)):
        sgn = np.array([1.0 if k & 1 else -1.0, 1.0 if k & 2 else -1.0])
        wall = np.where(sgn > 0, bc.P_MAX, bc.P_MIN)
        p0 = pr["C"] @ pr["x0"]
        assert np.all((wall - p0) * sgn >= 0.2 - 1e-12) and np.all((wall - p0) * sgn <= 0.8 + 1e-12)
        assert np.all((pr["x_ref"][-1, :2] - wall) * sgn >= 0.5)
        assert np.all(pr["x_ref"][:, 2:] == 0) and np.all(pr["x0"][2:] != 0)
        assert np.all(pr["u_ref"] != 0)


def test_mixed_batch_has_one_certified_problem_between_two_unreachable_ones():
    """tests/test_mpc_bounds_gpu.py's mixed batch: the oracle certifies problem 1 (it stays at its
    start inside the box); problems 0 and 2 would need to cover 8 in 10 steps of 0.2 with |u| <= 1
    (at most 0.5 * 2^2 = 2 from rest), so no input sequence reaches the box."""
    from test_mpc import _oracle
    prs = bc.mixed_batch()
    x, u, io = _oracle(prs[1])
    assert io["status"] == "optimal" and max(io["kkt"].values()) < 1e-8
    np.testing.assert_allclose(u, 0.0, atol=1e-9)
    for b in (0, 2):
        reach = 0.5 * np.max(np.abs(prs[b]["ub"])) * (prs[b]["H"] * 0.2) ** 2
        assert np.all(prs[b]["x0"] == 0) and reach < prs[b]["pb"][0].min()
    rows = [pr["u_ref"] for pr in prs]
    assert not any(np.array_equal(rows[i], rows[j]) for i in range(3) for j in range(i))
