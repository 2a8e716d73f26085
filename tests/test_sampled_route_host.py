"""CPU: the host side of the route library (include/drcvar_loop_route.h): the symbol lists, the
host checks of drcvar_sampled_halfspaces_f64_route and drcvar_mpc_step_advance_batch_route_f64,
ReferenceTrajectoryPlanner.straight_line_routes and the shape errors of a batch with a route per
problem.  Every call here returns or raises before any launch: no pointer is device memory and no
device is reached."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core.mpc_filter import MPCModel
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams, RiskTable
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import closed_loop
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.planner import (
    ReferenceTrajectoryPlanner)

INV, UNS, OK = _native.ERR_INVALID_ARGUMENT, _native.ERR_UNSUPPORTED, _native.OK
POINTERS = ("nominal_path", "state", "ego_path", "table", "metric", "out", "selected")
ADVANCE_POINTERS = ("x_out", "u_out", "info", "x_ref_path", "u_ref_path", "x_log", "u_log", "info_log",
                    "x0", "x_ref_win", "u_fallback", "last_u", "have_last", "state")


def _symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return set(re.findall(r"\bT (drcvar_\w+)", out))


def test_route_library_exports_what_its_header_declares():
    text = re.sub(r"/\*.*?\*/", "", open(_native.ROUTE_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(drcvar_\w+)\s*\(", text, flags=re.M)))
    assert declared == sorted(_native.ROUTE_SYMBOLS)
    assert declared == ["drcvar_mpc_step_advance_batch_route_f64", "drcvar_sampled_halfspaces_f64_route"]
    lib = _native.route_lib()
    assert _symbols(_native.ROUTE_LIB_PATH) == set(declared)
    assert b"gfx950" in open(_native.ROUTE_LIB_PATH, "rb").read()
    # the other six lists are what they were, and disjoint from the new one
    lists = (_native.EXPORTED_SYMBOLS, _native.LOOP_SYMBOLS, _native.EVAL_SYMBOLS, _native.PRED_SYMBOLS,
             _native.RISK_SYMBOLS, _native.METRIC_SYMBOLS)
    for other in lists:
        assert not set(declared) & set(other)
    for path, symbols in zip((_native.LIB_PATH, _native.LOOP_LIB_PATH, _native.EVAL_LIB_PATH,
                              _native.PRED_LIB_PATH, _native.RISK_LIB_PATH, _native.METRIC_LIB_PATH),
                             lists):
        assert _symbols(path) == set(symbols), path
    assert tuple(len(s) for s in lists) == (33, 1, 2, 1, 3, 2)
    assert _native.ABI_VERSION == 3
    # two objects, the two sources compiled once more with one define
    assert len(_native.ROUTE_UNIT) == 2
    (src0, defs0), (src1, defs1) = _native.ROUTE_UNIT
    assert src0 in _native.SOURCES and src0.endswith("drcvar_sampled.hip")
    assert src1 in _native.SOURCES and src1.endswith("drcvar_step.hip")
    assert defs0 == defs1 == ("-DDRCVAR_LOOP_ROUTE_LIBRARY",)
    # the argument lists: the metric entry's and the batch entry's with the strides inserted
    i64 = ctypes.c_int64
    route = lib.drcvar_sampled_halfspaces_f64_route.argtypes
    metric = _native.metric_lib().drcvar_sampled_halfspaces_f64_metric.argtypes
    assert len(route) == 26 and route == metric[:17] + [i64] + metric[17:]
    advance = lib.drcvar_mpc_step_advance_batch_route_f64.argtypes
    batch = _native.loop_lib().drcvar_mpc_step_advance_batch_f64.argtypes
    assert len(advance) == 23 and advance == batch[:8] + [i64, i64] + batch[8:]


# ---- the halfspace entry's host checks ---------------------------------------------------------------
def _call(lib, entry="route", **kw):
    """The entry with host values that pass every check unless ``kw`` says otherwise (the device
    pointers are the address 64: a launch would follow, so every case here must return first).
    ``entry="metric"``: the same arguments, without the problem stride, to the metric entry."""
    a = dict(nominal_path=64, BO=6, P=9, nom_so=18, nom_st=2, T=4, u0=0, count=24, n=100, l00=0.1,
             l10=0.0, l11=0.1, seed=1, state=64, zero_first=1, ego_path=64, ego_st=2, ego_ps=18, O=3,
             table=64, D=2, metric=64, out=64, status=64, selected=64)
    a.update(kw)
    vp = ctypes.c_void_p
    head = (vp(a["nominal_path"]), a["BO"], a["P"], a["nom_so"], a["nom_st"], a["T"], a["u0"], a["count"],
            a["n"], a["l00"], a["l10"], a["l11"], a["seed"], vp(a["state"]), a["zero_first"],
            vp(a["ego_path"]), a["ego_st"])
    tail = (a["O"], vp(a["table"]), a["D"], vp(a["metric"]), vp(a["out"]), vp(a["status"]),
            vp(a["selected"]), None)
    if entry == "metric":
        return lib.drcvar_sampled_halfspaces_f64_metric(*head, *tail)
    return lib.drcvar_sampled_halfspaces_f64_route(*head, a["ego_ps"], *tail)


def test_route_halfspace_host_validation():
    lib, metric = _native.route_lib(), _native.metric_lib()
    assert _call(lib, count=0) == OK                       # nothing to launch ...
    assert _call(lib, count=0, **{name: None for name in POINTERS}) == OK   # ... no pointer looked at
    assert _call(lib, n=0) == OK
    nan = float("nan")
    # everything the metric entry rejects, with its code, at several strides
    rejected = [dict(O=0), dict(O=-2), dict(D=0), dict(D=-1), dict(O=4),
                dict(u0=-1), dict(count=-1), dict(u0=25, count=0), dict(u0=1), dict(count=25),
                dict(u0=23, count=2),
                dict(BO=-6), dict(T=-1), dict(n=-1), dict(P=0), dict(P=-3), dict(l00=nan), dict(l10=nan),
                dict(l11=nan),
                dict(n=_native.MAX_SAMPLES + 1), dict(BO=3 * 2 ** 40, T=1, count=1),
                dict(n=_native.MAX_SAMPLES + 1, D=0), dict(count=0, O=0), dict(count=0, D=0)]
    rejected += [{name: None} for name in POINTERS]
    rejected += [dict(state=64 + off) for off in (1, 4, 8, 12)] + [dict(table=64 + off) for off in (1, 4, 8, 12)]
    for kw in rejected:
        want = _call(metric, "metric", **kw)
        assert want in (INV, UNS), kw
        for stride in (0, 18, 2 ** 40):
            assert _call(lib, ego_ps=stride, **kw) == want, (kw, stride)
    assert sum(_call(metric, "metric", **kw) == UNS for kw in rejected) == 2
    # the stride of its own
    for stride in (-1, -18, -2 ** 63):
        assert _call(lib, ego_ps=stride) == INV, stride
        assert _call(lib, ego_ps=stride, count=0) == INV, stride
    for stride in (2 ** 40 + 1, 2 ** 41, 2 ** 63 - 1):
        assert _call(lib, ego_ps=stride) == UNS, stride
    for stride in (0, 1, 18, 2 ** 40):
        assert _call(lib, ego_ps=stride, count=0) == OK, stride
    for null in ("metric", "selected"):
        assert _call(lib, **{null: None}, count=0) == OK, null
        assert _call(lib, **{null: None}, n=0) == OK, null
    assert _call(lib, status=None, count=0) == OK           # (status is optional)


# ---- the advance entry's host checks ------------------------------------------------------------------
def _model(horizon=4):
    dt = 0.2
    A = np.array([[1, 0, dt, 0], [0, 1, 0, dt], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    B = np.array([[0.5 * dt * dt, 0], [0, 0.5 * dt * dt], [dt, 0], [0, dt]], dtype=np.float64)
    C = np.array([[1, 0, 0, 0], [0, 1, 0, 0]], dtype=np.float64)
    return MPCModel(A, B, C, np.eye(4), 0.1 * np.eye(2), horizon, device="cpu")


def _advance(lib, mdl, **kw):
    a = {name: 64 for name in ADVANCE_POINTERS}
    a.update(model=ctypes.byref(mdl), B=3, P=9, xs=36, us=18, disturbance=None, step_begin=0, log_rows=5)
    a.update(kw)
    vp = ctypes.c_void_p
    return lib.drcvar_mpc_step_advance_batch_route_f64(
        a["model"], a["B"], vp(a["x_out"]), vp(a["u_out"]), vp(a["info"]), vp(a["x_ref_path"]),
        vp(a["u_ref_path"]), a["P"], a["xs"], a["us"], vp(a["disturbance"]), a["step_begin"],
        a["log_rows"], vp(a["x_log"]), vp(a["u_log"]), vp(a["info_log"]), vp(a["x0"]),
        vp(a["x_ref_win"]), vp(a["u_fallback"]), vp(a["last_u"]), vp(a["have_last"]), vp(a["state"]),
        None)


def test_route_advance_host_validation():
    lib = _native.route_lib()
    m = _model().model
    # the batch entry's checks, at any positive problem count and any stride
    for B, strides in ((1, (0, 0)), (3, (36, 18)), (2 ** 31 - 1, (2 ** 40, 2 ** 40))):
        kw = dict(B=B, xs=strides[0], us=strides[1])
        assert _advance(lib, m, model=None, **kw) == INV
        for null in ADVANCE_POINTERS:
            assert _advance(lib, m, **kw, **{null: None}) == INV, null
        for off in (1, 4, 8, 12):
            assert _advance(lib, m, state=64 + off, **kw) == INV, off
        assert _advance(lib, m, log_rows=-1, **kw) == INV
        assert _advance(lib, m, P=0, **kw) == INV and _advance(lib, m, P=-1, **kw) == INV
        for field, bad in (("horizon", 0), ("horizon", _native.MPC_MAX_HORIZON + 1), ("n_states", 0),
                           ("n_states", _native.MPC_MAX_STATES + 1), ("n_inputs", 0),
                           ("n_inputs", _native.MPC_MAX_INPUTS + 1)):
            broken = _native.MpcModel.from_buffer_copy(m)
            setattr(broken, field, bad)
            assert _advance(lib, broken, **kw) == INV, (field, bad)
    assert _advance(lib, m, B=-1) == INV and _advance(lib, m, B=-2 ** 63) == INV
    for B in (2 ** 31, 2 ** 40, 2 ** 63 - 1):
        assert _advance(lib, m, B=B) == UNS, B
        assert _advance(lib, m, B=B, state=None) == INV   # an invalid call stays invalid
    # the strides of its own, each alone
    for name in ("xs", "us"):
        for stride in (-1, -36, -2 ** 63):
            assert _advance(lib, m, **{name: stride}) == INV, (name, stride)
        for stride in (2 ** 40 + 1, 2 ** 41, 2 ** 63 - 1):
            assert _advance(lib, m, **{name: stride}) == UNS, (name, stride)
    assert _advance(lib, m, xs=-1, us=2 ** 41) == INV
    # nothing to do: no launch, no other argument is looked at
    assert _advance(lib, m, B=0) == OK
    assert _advance(lib, m, B=0, model=None, xs=-1, us=2 ** 41,
                    **{name: None for name in ADVANCE_POINTERS}) == OK


# ---- the Python surface ----------------------------------------------------------------------------------
def test_straight_line_routes_stack_the_single_call():
    m = _model(horizon=10)
    planner = ReferenceTrajectoryPlanner(m.A, m.B, m.C, np.eye(4), 0.1 * np.eye(2), 10, 0.2)
    starts = np.array([[0.0, 0.0], [0.5, -0.25], [0.0, 0.0], [1.0, 1.0]])
    goals = np.array([[4.0, 0.0], [4.0, 1.0], [3.0, -1.0], [1.0, 1.0]])       # (the last: no motion)
    speeds = np.array([1.5, 1.5, 1.0, 0.7])
    x_ref, u_ref = planner.straight_line_routes(starts, goals, speeds)
    assert x_ref.shape == (4, 11, 4) and u_ref.shape == (4, 10, 2)
    assert x_ref.dtype == u_ref.dtype == np.float64
    for b in range(4):
        x, u, _ = planner.straight_line_trajectory(starts[b], goals[b], speeds[b])
        assert x_ref[b].tobytes() == x.tobytes() and u_ref[b].tobytes() == u.tobytes(), b
    # the arguments broadcast against each other
    x1, u1 = planner.straight_line_routes(starts[0], goals, 1.5)
    for b in range(4):
        x, u, _ = planner.straight_line_trajectory(starts[0], goals[b], 1.5)
        assert x1[b].tobytes() == x.tobytes() and u1[b].tobytes() == u.tobytes(), b
    x2, u2 = planner.straight_line_routes(starts[0], goals[1], speeds)
    for b in range(4):
        x, u, _ = planner.straight_line_trajectory(starts[0], goals[1], speeds[b])
        assert x2[b].tobytes() == x.tobytes() and u2[b].tobytes() == u.tobytes(), b
    x3, u3 = planner.straight_line_routes(starts[0], goals[0])                # three scalars: B = 1
    x, u, _ = planner.straight_line_trajectory(starts[0], goals[0], 1.5)
    assert x3.shape == (1, 11, 4) and x3[0].tobytes() == x.tobytes() and u3[0].tobytes() == u.tobytes()
    for bad in ((starts[:3], goals, 1.5), (starts, goals, speeds[:2]), (starts[:, :1], goals, 1.5),
                (starts, goals[None], 1.5), (starts, goals, speeds[None])):
        with pytest.raises(ValueError):
            planner.straight_line_routes(*bad)


def test_batch_rejects_route_shapes_before_the_device():
    m = _model()
    f64 = torch.float64
    B, O, P = 3, 2, 9
    nominal = torch.zeros((B, O, P, 2), dtype=f64)
    x2, u2 = torch.zeros((P, 4), dtype=f64), torch.zeros((P, 2), dtype=f64)
    x3, u3 = torch.zeros((B, P, 4), dtype=f64), torch.zeros((B, P, 2), dtype=f64)

    def batch(x_ref, u_ref, params=RiskParams(), **kw):
        return closed_loop.RecedingHorizonBatch(m, nominal, x_ref, u_ref, 100, params, n_problems=B, **kw)

    for rows in (1, 2, 4):                                  # a first dimension that is not B
        with pytest.raises(ValueError, match="n_problems"):
            batch(torch.zeros((rows, P, 4), dtype=f64), u2)
        with pytest.raises(ValueError, match="n_problems"):
            batch(x2, torch.zeros((rows, P, 2), dtype=f64))
        with pytest.raises(ValueError, match="n_problems"):
            batch(x3, torch.zeros((rows, P, 2), dtype=f64))
    for bad_x, bad_u in ((torch.zeros((B, P - 1, 4), dtype=f64), u3), (torch.zeros((B, P, 3), dtype=f64), u3),
                         (x3, torch.zeros((B, P + 1, 2), dtype=f64)), (x3, torch.zeros((B, P, 3), dtype=f64)),
                         (x3.float(), u3), (torch.zeros((1, B, P, 4), dtype=f64), u3)):
        with pytest.raises(ValueError, match="x_ref_path|u_ref_path"):
            batch(bad_x, bad_u)
    # what a route batch takes beside its paths is checked as the metric batch checks it
    with pytest.raises(ValueError, match="rows"):
        batch(x3, u3, RiskTable(epsilon=[0.0, 0.1]))
    with pytest.raises(ValueError, match="names"):
        batch(x3, u3, metric=["mean", "cvar"])
    for D in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="draw_period"):
            batch(x3, u3, draw_period=D)
    with pytest.raises(ValueError, match="predicted"):      # a table stays out of the predicted form
        batch(x3, u3, RiskTable(epsilon=[0.0, 0.1, 0.2]), linearize="predicted")
    with pytest.raises(ValueError, match="draw_period"):    # ... and a draw period with it
        batch(x3, u3, linearize="predicted", draw_period=1)
    with pytest.raises(ValueError, match="metric"):
        batch(x3, u3, metric="median")
    # host tensors of the right shapes reach the device check, 2-D and 3-D alike
    for x_ref, u_ref in ((x3, u3), (x3, u2), (x2, u3), (x2, u2)):
        with pytest.raises(ValueError, match="GPU"):
            batch(x_ref, u_ref)


def test_engine_rejects_a_wrong_route_ego_path():
    f64 = torch.float64
    B, O, T, P = 3, 2, 4, 9
    nominal = torch.zeros((B * O, P, 2), dtype=f64)
    state = torch.zeros(2, dtype=torch.int64)
    table = RiskTable(epsilon=[0.0, 0.1, 0.2])
    names = ("mean", "cvar", "dr_cvar")

    def prepare(ego, **kw):
        return engine.prepare_sampled_halfspaces_route(nominal, ego, O, T, 100, table, names, state, **kw)

    for shape in ((P, 2), (B + 1, P, 2), (B, P + 1, 2), (B, P, 3), (B, P), (1, B, P, 2)):
        with pytest.raises(ValueError, match="ego_path"):
            prepare(torch.zeros(shape, dtype=f64))
    with pytest.raises(ValueError, match="ego_path"):
        prepare(torch.zeros((B, P, 2), dtype=torch.float32))
    with pytest.raises(ValueError, match="ego_path"):      # coordinates adjacent
        prepare(torch.zeros((B, P, 4), dtype=f64)[:, :, ::2])
    with pytest.raises(ValueError, match="metric"):
        engine.prepare_sampled_halfspaces_route(nominal, torch.zeros((B, P, 2), dtype=f64), O, T, 100,
                                                table, names[:2], state)
    with pytest.raises(ValueError, match="GPU"):           # (host tensors: no CPU path)
        prepare(torch.zeros((B, P, 2), dtype=f64))
    # check_path takes the 3-D shape, strided in both leading dimensions
    wide = torch.zeros((B, 2 * P, 3), dtype=f64)[:, ::2, :2]
    with pytest.raises(ValueError, match="GPU"):
        engine.check_path(wide, "ego_path", (B, P, 2))
    with pytest.raises(ValueError, match="shape"):
        engine.check_path(wide, "ego_path", (B + 1, P, 2))
