"""Safety-filter QPs whose boxes bind, for tests/test_mpc_bounds_host.py and
tests/test_mpc_bounds_gpu.py: plain NumPy on top of tests/test_mpc.py's `_random_problem` and the
oracle (oracle/mpc_qp.py), never the product path.

`_random_problem` gives every input the box +-1.5 and both position axes +-4, with halfspaces about
the origin that hold the path away from the position box, and either both boxes or none.  Here

* a problem has the input box alone (form "u"), the position box alone ("p") or both ("up");
* every bound is its own number: u_min[i] = -k_u (0.6 + 0.35 i), u_max[i] = k_u (1.1 + 0.3 i),
  p_min = (-3.5, -2.5), p_max = (2.0, 4.5) — no two equal in absolute value, so a kernel that read
  another component's bound, the other side's negated or the other axis's gives another answer;
* problem k starts inside the position box near its corner k mod 4, with a start velocity where
  the model has one, and its reference leaves the box through that corner, so the box holds the
  optimum; the halfspaces lie about the reference clipped to the box (about one row in six
  violated there: some slacks positive, some rows active at zero slack); u_ref (the fallback
  inputs; the objective does not see them) is not zero.

All problems of a case share the model and go in one launch.  tests/test_mpc_bounds_host.py holds
the conditions — every side of every bounded component active in some problem of the case, every
problem KKT-certified — without which the device tests would compare idle rows.
"""
import numpy as np

from test_mpc import _oracle, _random_problem, double_integrator

P_MIN = np.array([-3.5, -2.5])
P_MAX = np.array([2.0, 4.5])
ACTIVE_TOL = 1e-9            # |value - bound| on the oracle's optimum

FORMS = ("u", "p", "up")
# (dyn, H, O): every input width (1, 2, 3, 4) and state template (2, 3, 4, 5, 8 states)
FEW = [("double", 12, 3), ("single", 9, 2), ("generic3", 10, 3), ("generic44", 8, 2),
       ("generic4", 8, 2), ("generic8", 8, 2), ("drag", 12, 3), ("double_full", 12, 3),
       ("double", 33, 3)]
FEW_ONE_INPUT = [("generic1", 16, 2)]   # one input cannot hold a two-dimensional box: form "u" only
MANY = [("double", 12, 3), ("generic8", 8, 2), ("double", 33, 3)]   # 128 threads; 256 at H > 32
CLUSTER = [("double", 12, 64), ("generic3", 10, 64), ("generic8", 8, 64)]  # rows in LDS; in memory
N_FEW, N_MANY, N_CLUSTER = 16, 144, 8
HOST_PROBLEMS = 16           # the host conditions look at the first 16 problems of a many case

# (group, dyn, H, O, form, problems per launch)
CASES = ([("few", *c, f, N_FEW) for c in FEW for f in FORMS]
         + [("few", *c, "u", N_FEW) for c in FEW_ONE_INPUT]
         + [("many", *c, f, N_MANY) for c in MANY for f in FORMS]
         + [("cluster", *c, f, N_CLUSTER) for c in CLUSTER for f in FORMS])


def case_id(case):
    group, dyn, H, O, form, n = case
    return f"{group}-{dyn}-H{H}-O{O}-{form}"


def input_box(nu):
    """(u_min, u_max).  Wide input sets are over-actuated: with the full box some inputs never
    saturate, so three and more inputs get the box scaled by 0.3."""
    k_u = 1.0 if nu <= 2 else 0.3
    i = np.arange(nu)
    return -k_u * (0.6 + 0.35 * i), k_u * (1.1 + 0.3 * i)


def bound_problem(rng, base, form, k):
    """Problem k of a case: `base` (a `_random_problem`) supplies A, B, C, Q, R and H."""
    A, B, C, H = base["A"], base["B"], base["C"], base["H"]
    nx, nu = A.shape[0], B.shape[1]
    O = base["hs"].shape[0]
    sgn = np.array([1.0 if k & 1 else -1.0, 1.0 if k & 2 else -1.0])
    wall = np.where(sgn > 0, P_MAX, P_MIN)
    p0 = wall - sgn * rng.uniform(0.2, 0.8, 2)
    x0 = np.linalg.pinv(C) @ p0
    if nx >= 4:
        x0[2:4] += rng.uniform(-0.3, 0.3, 2)
    ramp = np.minimum(1.0, np.arange(H + 1) / max(1, H // 2))
    x_ref = np.zeros((H + 1, nx))
    x_ref[:, :2] = p0 + np.outer(ramp, (wall - p0) + sgn * rng.uniform(0.5, 1.5, 2))
    u_ref = rng.uniform(-0.3, 0.3, (H, nu))
    ang = rng.uniform(0, 2 * np.pi, (O, H))
    h = np.stack([np.cos(ang), np.sin(ang)], -1)
    centre = np.clip(x_ref[1:, :2], P_MIN, P_MAX)              # the box's numbers in every form
    g = -np.einsum("otc,tc->ot", h, centre) - rng.normal(0.6, 0.6, (O, H))
    pr = dict(base)
    pr.update(x0=x0, x_ref=x_ref, u_ref=u_ref, hs=np.concatenate([h, g[..., None]], -1),
              ub=input_box(nu) if "u" in form else None,
              pb=(P_MIN.copy(), P_MAX.copy()) if "p" in form else None)
    return pr


_PROBLEMS = {}
_ORACLE = {}


def problems(case):
    """The case's problems, generated once; a many case's first problems are drawn like the rest."""
    if case not in _PROBLEMS:
        group, dyn, H, O, form, n = case
        rng = np.random.default_rng([H, O, len(form), sum(map(ord, dyn))] + SEED_EXTRA.get(case[1:5], []))
        base = _random_problem(rng, O, H, H, dyn)
        _PROBLEMS[case] = [bound_problem(rng, base, form, k) for k in range(n)]
    return _PROBLEMS[case]


# With the plain seed one side stays idle in two cases (p_min[0] in the first, u_max[1] in the
# second: tests/test_mpc_bounds_host.py would fail); these extra seed words give every side >= 2.
SEED_EXTRA = {("generic8", 8, 2, "up"): [3], ("generic8", 8, 64, "up"): [2]}


def oracle(case, k):
    """(x, u, info) of the oracle on problem k of the case, computed once and left unchanged.  A
    few and a many case of one (dyn, H, O, form) draw the same stream, so they share problems."""
    key = case[1:5] + (k,)
    if key not in _ORACLE:
        _ORACLE[key] = _oracle(problems(case)[k])
    return _ORACLE[key]


def oracle_subset(case):
    """The problems of a case that are compared with the oracle: all of a few or cluster case; of
    a many case the first 16, the last one and every ninth in between."""
    n = case[5]
    return list(range(n)) if case[0] != "many" else list(range(16)) + list(range(16, n - 1, 9)) + [n - 1]


def mixed_batch():
    """Three problems of tests/test_mpc.py's infeasible model (H = 10, |u| <= 1, position box
    [8, 9]^2, no halfspaces): 0 and 2 start at the origin and cannot reach the box, 1 starts inside
    it at (8.5, 8.5) with its reference constant there.  Each has its own random fallback inputs."""
    A, B, C = double_integrator()
    H = 10
    rng = np.random.default_rng(23)
    prs = []
    for k in range(3):
        x0 = np.array([8.5, 8.5, 0.0, 0.0]) if k == 1 else np.zeros(4)
        prs.append(dict(A=A, B=B, C=C, Q=2 * np.eye(4), R=np.eye(2), H=H, x0=x0,
                        x_ref=np.tile(x0, (H + 1, 1)), u_ref=rng.uniform(-0.5, 0.5, (H, 2)),
                        hs=np.zeros((0, H, 3)), ub=(np.full(2, -1.0), np.full(2, 1.0)),
                        pb=(np.full(2, 8.0), np.full(2, 9.0))))
    return prs


def bound_values(pr):
    """All 2 nu + 4 bound values the generator can use for this model (a form selects among them)."""
    lo, hi = input_box(pr["B"].shape[1])
    return np.concatenate([lo, hi, P_MIN, P_MAX])


def active_sides(pr, x, u, tol):
    """The set of (kind, t, component, side) at which the answer touches a bound within `tol`:
    kind "u" with t = 0..H-1, kind "p" with t = 1..H; side 0 = min, 1 = max."""
    out = set()
    if pr["ub"] is not None:
        for side, b in enumerate(pr["ub"]):
            out |= {("u", int(t), int(i), side) for t, i in zip(*np.nonzero(np.abs(u - b) < tol))}
    if pr["pb"] is not None:
        p = x[1:] @ pr["C"].T
        for side, b in enumerate(pr["pb"]):
            out |= {("p", int(t) + 1, int(i), side) for t, i in zip(*np.nonzero(np.abs(p - b) < tol))}
    return out


def side_counts(case, n=None):
    """{(kind, component, side): problems of the case whose oracle optimum has that side active}."""
    prs = problems(case)[:n]
    counts = {}
    for kind, dim in (("u", prs[0]["B"].shape[1] if prs[0]["ub"] is not None else 0),
                      ("p", 2 if prs[0]["pb"] is not None else 0)):
        for i in range(dim):
            for side in (0, 1):
                counts[kind, i, side] = 0
    for k, pr in enumerate(prs):
        x, u, _ = oracle(case, k)
        for key in {(kind, i, side) for kind, _, i, side in active_sides(pr, x, u, ACTIVE_TOL)}:
            counts[key] += 1
    return counts


def halfspace_residuals(pr, x):
    """h . C x_{k+1} + g of every row, [O, H]."""
    p = x[1:] @ pr["C"].T
    return np.einsum("otc,tc->ot", pr["hs"][..., :2], p) + pr["hs"][..., 2]
