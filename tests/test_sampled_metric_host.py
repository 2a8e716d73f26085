"""CPU: the host side of the metric library (include/drcvar_loop_metric.h): the symbol lists, the
host checks of drcvar_sampled_halfspaces_f64_metric and the metric=[...] surface of the engine and
the loop classes.  Every call here returns or raises before any launch: no pointer is device memory
and no device is reached."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core.mpc_filter import (
    METRIC_COLUMNS, MPCModel)
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams, RiskTable
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import closed_loop

INV, UNS, OK = _native.ERR_INVALID_ARGUMENT, _native.ERR_UNSUPPORTED, _native.OK
POINTERS = ("nominal_path", "state", "ego_path", "table", "metric", "out", "selected")


def _symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return set(re.findall(r"\bT (drcvar_\w+)", out))


def test_metric_library_exports_what_its_header_declares():
    text = re.sub(r"/\*.*?\*/", "", open(_native.METRIC_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(drcvar_\w+)\s*\(", text, flags=re.M)))
    assert declared == sorted(_native.METRIC_SYMBOLS)
    assert declared == ["drcvar_metric_table_row_bytes", "drcvar_sampled_halfspaces_f64_metric"]
    lists = (_native.EXPORTED_SYMBOLS, _native.LOOP_SYMBOLS, _native.EVAL_SYMBOLS, _native.PRED_SYMBOLS,
             _native.RISK_SYMBOLS)
    for other in lists:
        assert not set(declared) & set(other)
    lib = _native.metric_lib()
    assert _symbols(_native.METRIC_LIB_PATH) == set(declared)
    assert b"gfx950" in open(_native.METRIC_LIB_PATH, "rb").read()
    assert len(lib.drcvar_sampled_halfspaces_f64_metric.argtypes) == 25
    # the other five libraries export what they did
    for path, symbols in zip((_native.LIB_PATH, _native.LOOP_LIB_PATH, _native.EVAL_LIB_PATH,
                              _native.PRED_LIB_PATH, _native.RISK_LIB_PATH), lists):
        assert _symbols(path) == set(symbols), path
    assert tuple(len(s) for s in lists) == (33, 1, 2, 1, 3)
    assert _native.ABI_VERSION == 3
    # the same source, compiled once more with a define of its own
    src, defs = _native.METRIC_UNIT
    assert src in _native.SOURCES and src.endswith("drcvar_sampled.hip")
    assert defs == ("-DDRCVAR_LOOP_METRIC_LIBRARY",)


def test_header_constants_and_row_bytes():
    text = open(_native.METRIC_HEADER).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define (DRCVAR_(?:METRIC|SEL)_\w+) (-?\d+)$", text, flags=re.M)}
    assert defines == dict(DRCVAR_METRIC_MEAN=0, DRCVAR_METRIC_CVAR=1, DRCVAR_METRIC_DR_CVAR=2,
                           DRCVAR_SEL_H0=0, DRCVAR_SEL_H1=1, DRCVAR_SEL_G=2, DRCVAR_SEL_WIDTH=4)
    assert engine.METRIC_CODES == {"mean": 0, "cvar": 1, "dr_cvar": 2}
    assert set(engine.METRIC_CODES) == set(METRIC_COLUMNS) and engine.SELECTED_WIDTH == 4
    row = int(_native.metric_lib().drcvar_metric_table_row_bytes())
    assert row == int(_native.risk_lib().drcvar_risk_table_row_bytes()) and row % 16 == 0


# ---- the launch entry's host checks ----------------------------------------------------------------
def _call(lib, entry="metric", **kw):
    """The entry with host values that pass every check unless ``kw`` says otherwise (the device
    pointers are the address 64: a launch would follow, so every case here must return first).
    ``entry="risk"``: the same arguments to the risk-table entry."""
    a = dict(nominal_path=64, BO=6, P=9, nom_so=18, nom_st=2, T=4, u0=0, count=24, n=100, l00=0.1,
             l10=0.0, l11=0.1, seed=1, state=64, zero_first=1, ego_path=64, ego_st=2, O=3, table=64,
             D=2, metric=64, out=64, status=64, selected=64)
    a.update(kw)
    vp = ctypes.c_void_p
    head = (vp(a["nominal_path"]), a["BO"], a["P"], a["nom_so"], a["nom_st"], a["T"], a["u0"], a["count"],
            a["n"], a["l00"], a["l10"], a["l11"], a["seed"], vp(a["state"]), a["zero_first"],
            vp(a["ego_path"]), a["ego_st"], a["O"], vp(a["table"]), a["D"])
    if entry == "risk":
        return lib.drcvar_sampled_halfspaces_f64_risk(*head, vp(a["out"]), vp(a["status"]), None)
    return lib.drcvar_sampled_halfspaces_f64_metric(*head, vp(a["metric"]), vp(a["out"]), vp(a["status"]),
                                                    vp(a["selected"]), None)


def test_host_validation():
    lib, risk = _native.metric_lib(), _native.risk_lib()
    assert _call(lib, count=0) == OK                       # nothing to launch ...
    assert _call(lib, count=0, **{name: None for name in POINTERS}) == OK   # ... no pointer looked at
    assert _call(lib, n=0) == OK
    nan = float("nan")
    # everything the risk-table entry rejects, with its code
    rejected = [dict(O=0), dict(O=-2), dict(D=0), dict(D=-1), dict(O=4),
                dict(u0=-1), dict(count=-1), dict(u0=25, count=0), dict(u0=1), dict(count=25),
                dict(u0=23, count=2),
                dict(BO=-6), dict(T=-1), dict(n=-1), dict(P=0), dict(P=-3), dict(l00=nan), dict(l10=nan),
                dict(l11=nan),
                dict(n=_native.MAX_SAMPLES + 1), dict(BO=3 * 2 ** 40, T=1, count=1),
                dict(n=_native.MAX_SAMPLES + 1, D=0), dict(count=0, O=0), dict(count=0, D=0)]
    rejected += [{name: None} for name in POINTERS if name not in ("metric", "selected")]
    rejected += [dict(state=64 + off) for off in (1, 4, 8, 12)] + [dict(table=64 + off) for off in (1, 4, 8, 12)]
    for kw in rejected:
        want = _call(risk, "risk", **kw)
        assert want in (INV, UNS), kw
        assert _call(lib, **kw) == want, kw
    assert sum(_call(risk, "risk", **kw) == UNS for kw in rejected) == 2
    # the two pointers of its own, null pointer by null pointer
    for null in ("metric", "selected"):
        assert _call(lib, **{null: None}) == INV, null
        assert _call(lib, **{null: None}, count=0) == OK, null
        assert _call(lib, **{null: None}, n=0) == OK, null
    assert _call(lib, status=None, count=0) == OK           # (status is optional)
    assert _call(lib, table=64 + 5, count=0) == OK          # (nothing launched: the table is not read)
    for D in (1, 2, 3, 2 ** 40):
        assert _call(lib, D=D, count=0) == OK


# ---- the Python surface ----------------------------------------------------------------------------
def _model(horizon=4):
    dt = 0.2
    A = np.array([[1, 0, dt, 0], [0, 1, 0, dt], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    B = np.array([[0.5 * dt * dt, 0], [0, 0.5 * dt * dt], [dt, 0], [0, dt]], dtype=np.float64)
    C = np.array([[1, 0, 0, 0], [0, 1, 0, 0]], dtype=np.float64)
    return MPCModel(A, B, C, np.eye(4), 0.1 * np.eye(2), horizon, device="cpu")


def test_constructors_reject_bad_metric_arguments_before_the_device():
    m = _model()
    f64 = torch.float64
    nominal, x_ref, u_ref = torch.zeros((3, 2, 9, 2), dtype=f64), torch.zeros((9, 4), dtype=f64), \
        torch.zeros((9, 2), dtype=f64)
    table = RiskTable(epsilon=[0.0, 0.1, 0.2])
    names = ["mean", "cvar", "dr_cvar"]

    def batch(metric, params=RiskParams(), **kw):
        return closed_loop.RecedingHorizonBatch(m, nominal, x_ref, u_ref, 100, params, n_problems=3,
                                                metric=metric, **kw)

    for params in (RiskParams(), table):
        with pytest.raises(ValueError, match="names"):                 # a length that is not B
            batch(names[:2], params)
        with pytest.raises(ValueError, match="names"):
            batch(names + ["mean"], params)
        with pytest.raises(ValueError, match="names"):
            batch([], params)
        for bad in ("var", "", None, 2):                               # an unknown name
            with pytest.raises(ValueError, match="names"):
                batch(["mean", bad, "cvar"], params)
        with pytest.raises(ValueError, match="predicted"):
            batch(names, params, linearize="predicted")
        with pytest.raises(ValueError, match="RecedingHorizonBatch"):  # the single-loop class
            closed_loop.RecedingHorizonFilter(m, nominal[0], x_ref, u_ref, 100, RiskParams(), metric=names[:1])
    with pytest.raises(ValueError, match="RecedingHorizonBatch"):
        closed_loop.RecedingHorizonFilter(m, nominal[0], x_ref, u_ref, 100, RiskParams(), metric=tuple(names))
    for bad in ("var", 3, None):                                       # a single metric that is no name
        with pytest.raises(ValueError, match="metric"):
            batch(bad)
    for D in (0, -1, 1.5, True):                                       # draw_period beside a sequence
        with pytest.raises(ValueError, match="draw_period"):
            batch(names, draw_period=D)
    with pytest.raises(ValueError, match="rows"):
        batch(names, RiskTable(epsilon=[0.0, 0.1]))
    # a string metric with a RiskParams and a draw_period stays the error it is
    with pytest.raises(ValueError, match="draw_period"):
        batch("dr_cvar", draw_period=1)
    # the check itself
    assert closed_loop.check_metric("cvar", 3, "reference") is None
    assert closed_loop.check_metric("cvar", None, "predicted") is None
    assert closed_loop.check_metric(names, 3, "reference") == tuple(names)
    assert closed_loop.check_metric(iter(names), 3, "reference") == tuple(names)


def test_engine_rejects_a_wrong_metric_and_selected():
    f64 = torch.float64
    B, O, T, P = 3, 2, 4, 9
    nominal, ego = torch.zeros((B * O, P, 2), dtype=f64), torch.zeros((P, 2), dtype=f64)
    state = torch.zeros(2, dtype=torch.int64)
    table = RiskTable(epsilon=[0.0, 0.1, 0.2])
    names = ("mean", "cvar", "dr_cvar")

    def prepare(metric=names, **kw):
        return engine.prepare_sampled_halfspaces_metric(nominal, ego, O, T, 100, table, metric, state, **kw)

    for bad in (names[:2], names + ("mean",), (), "cvar"):
        with pytest.raises(ValueError, match="metric"):
            prepare(bad)
    with pytest.raises(ValueError, match="names"):
        prepare(("mean", "var", "cvar"))
    for shape in ((B * O, T, 8), (B * O, T), (B * O * T, 4), (B * O, T + 1, 4)):
        with pytest.raises(ValueError, match="selected"):
            prepare(selected=torch.zeros(shape, dtype=f64))
    with pytest.raises(ValueError, match="selected"):
        prepare(selected=torch.zeros((B * O, T, 4), dtype=torch.float32))
    with pytest.raises(ValueError, match="selected"):                  # a unit window: [units, 4]
        prepare(unit_begin=5, unit_count=7, selected=torch.zeros((B * O, T, 4), dtype=f64))
    for codes in (torch.zeros(B + 1, dtype=torch.int32), torch.zeros(B, dtype=torch.int64),
                  torch.zeros((B, 1), dtype=torch.int32)):
        with pytest.raises(ValueError, match="codes"):
            prepare(codes=codes)
    with pytest.raises(ValueError, match="RiskTable"):
        engine.prepare_sampled_halfspaces_metric(nominal, ego, O, T, 100, RiskParams(), names, state)
    with pytest.raises(ValueError, match="GPU"):                       # (host tensors: no CPU path)
        prepare(selected=torch.zeros((B * O, T, 4), dtype=f64), codes=torch.zeros(B, dtype=torch.int32))
    out, selected = torch.zeros((B * O, T, 8), dtype=f64), torch.zeros((B * O, T, 4), dtype=f64)
    codes = engine.metric_codes(names, B, "cpu")
    assert codes.dtype == torch.int32 and codes.tolist() == [0, 1, 2]
    h, g = engine.selected_views(selected, B, O)
    assert tuple(h.shape) == (B, O, T, 2) and tuple(g.shape) == (B, O, T)
    assert h.data_ptr() == selected.data_ptr() and g.data_ptr() == selected.data_ptr() + 16
    assert h.stride() == (O * T * 4, T * 4, 4, 1) and g.stride() == (O * T * 4, T * 4, 4)
    with pytest.raises(ValueError, match="selected"):
        engine.selected_views(out, B, O)
