"""CPU: the host side of the risk-table library (include/drcvar_loop_risk.h): the symbol lists,
drcvar_risk_table_fill, the host checks of drcvar_sampled_halfspaces_f64_risk, engine.RiskTable and
the params= / draw_period= surface of the loop classes.  Every call here returns or raises before
any launch: no pointer is device memory and no device is reached."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core.mpc_filter import MPCModel
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams, RiskTable
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import closed_loop

INV, UNS, OK = _native.ERR_INVALID_ARGUMENT, _native.ERR_UNSUPPORTED, _native.OK
POINTERS = ("nominal_path", "state", "ego_path", "table", "out")
FILL = 0xA5


def _symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return set(re.findall(r"\bT (drcvar_\w+)", out))


def test_risk_library_exports_what_its_header_declares():
    text = re.sub(r"/\*.*?\*/", "", open(_native.RISK_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(drcvar_\w+)\s*\(", text, flags=re.M)))
    assert declared == sorted(_native.RISK_SYMBOLS)
    assert declared == ["drcvar_risk_table_fill", "drcvar_risk_table_row_bytes",
                        "drcvar_sampled_halfspaces_f64_risk"]
    lists = (_native.EXPORTED_SYMBOLS, _native.LOOP_SYMBOLS, _native.EVAL_SYMBOLS, _native.PRED_SYMBOLS)
    for other in lists:
        assert not set(declared) & set(other)
    lib = _native.risk_lib()
    assert _symbols(_native.RISK_LIB_PATH) == set(declared)
    assert b"gfx950" in open(_native.RISK_LIB_PATH, "rb").read()
    assert len(lib.drcvar_sampled_halfspaces_f64_risk.argtypes) == 23
    # the other four libraries export what they did
    for path, symbols in zip((_native.LIB_PATH, _native.LOOP_LIB_PATH, _native.EVAL_LIB_PATH,
                              _native.PRED_LIB_PATH), lists):
        assert _symbols(path) == set(symbols), path
    assert tuple(len(s) for s in lists) == (33, 1, 2, 1)
    assert _native.ABI_VERSION == 3
    # the same source, compiled once more with a define of its own
    src, defs = _native.RISK_UNIT
    assert src in _native.SOURCES and src.endswith("drcvar_sampled.hip")
    assert defs == ("-DDRCVAR_LOOP_RISK_LIBRARY",)


# ---- drcvar_risk_table_fill ------------------------------------------------------------------------
def _fill(alpha, delta, epsilon, n_problems=None, rr=0.3, ro=0.3, n=100, rows=None, short=0,
          null=()):
    """(code, buffer [rows, row_bytes] between two guard rows, all pre-filled with FILL)."""
    lib = _native.risk_lib()
    row = int(lib.drcvar_risk_table_row_bytes())
    cols = [np.ascontiguousarray(np.asarray(v, dtype=np.float64)) for v in (alpha, delta, epsilon)]
    B = cols[0].shape[0] if n_problems is None else n_problems
    rows = max(B, 0) if rows is None else rows
    buf = np.full((rows + 2, row), FILL, dtype=np.uint8)
    ptrs = {name: c.ctypes.data for name, c in zip(("alpha", "delta", "epsilon"), cols)}
    ptrs["table"] = buf[1:].ctypes.data
    for name in null:
        ptrs[name] = None
    code = lib.drcvar_risk_table_fill(ptrs["alpha"], ptrs["delta"], ptrs["epsilon"], B, rr, ro, n,
                                      ptrs["table"], rows * row - short)
    return code, buf


def _untouched(buf):
    return bool(np.all(buf == FILL))


def test_row_bytes():
    row = int(_native.risk_lib().drcvar_risk_table_row_bytes())
    assert row > 0 and row % 16 == 0
    assert row >= 16 * 8        # at least the sixteen words of the launch-uniform scalars


def test_fill_writes_exactly_its_rows():
    alpha, delta, eps = [0.2, 0.2, 0.3, 0.2], [0.1, 0.1, 0.1, -0.1], [0.15, 0.15, 0.15, 0.3]
    code, buf = _fill(alpha, delta, eps, rows=6)
    assert code == OK
    assert _untouched(buf[0]) and _untouched(buf[5:])           # the guard and the two spare rows
    rows = buf[1:5]
    assert rows[0].tobytes() == rows[1].tobytes()               # equal triples: equal bytes
    for other in (2, 3):
        assert rows[0].tobytes() != rows[other].tobytes()
    # rows that differ in epsilon alone differ
    code, buf = _fill([0.2, 0.2], [0.1, 0.1], [0.15, 0.16])
    assert code == OK and buf[1].tobytes() != buf[2].tobytes()
    # filling again gives the same bytes (the padding is written too)
    again = _fill(alpha, delta, eps, rows=6)[1]
    assert again.tobytes() == _fill(alpha, delta, eps, rows=6)[1].tobytes()
    # a row depends on n_samples: the rank, 1 / k and the plan's window
    a = _fill([0.2], [0.1], [0.15], n=100)[1]
    for n in (101, 200, 1000, 2048):
        assert a.tobytes() != _fill([0.2], [0.1], [0.15], n=n)[1].tobytes(), n


def test_fill_return_codes():
    ok = ([0.2, 0.5], [0.1, 0.0], [0.15, 0.0])
    assert _fill(*ok)[0] == OK
    # legal rows: the kernel's UNBOUNDED and DR_UNBOUNDED exits, delta of either sign
    code, buf = _fill([1.5, 1.0, 0.2], [0.1, -0.1, 0.1], [0.15, 0.15, -0.1])
    assert code == OK and not np.any(np.all(buf[1:4] == FILL, axis=1))
    nan, inf = float("nan"), float("inf")
    rejected = [([0.2, 0.0], [0.1, 0.1], [0.1, 0.1]), ([0.2, -0.5], [0.1, 0.1], [0.1, 0.1]),
                ([0.2, nan], [0.1, 0.1], [0.1, 0.1]), ([inf, 0.2], [0.1, 0.1], [0.1, 0.1]),
                ([0.2, 0.2], [0.1, nan], [0.1, 0.1]), ([0.2, 0.2], [0.1, 0.1], [0.1, -inf]),
                ([0.2, 0.2], [0.1, 0.1], [nan, 0.1])]
    for triple in rejected:     # (the bad row is the second as often as the first: nothing written)
        code, buf = _fill(*triple)
        assert code == INV and _untouched(buf), triple
    for kw in (dict(rr=nan), dict(ro=inf)):
        code, buf = _fill(*ok, **kw)
        assert code == INV and _untouched(buf), kw
    # the buffer: too small by one byte, by a row, and absent
    for kw in (dict(short=1), dict(rows=1), dict(null=("table",)), dict(null=("alpha",)),
               dict(null=("delta",)), dict(null=("epsilon",)), dict(n_problems=-1)):
        code, buf = _fill(*ok, **kw)
        assert code == INV and _untouched(buf), kw
    for n in (0, -1, _native.MAX_SAMPLES + 1):
        code, buf = _fill(*ok, n=n)
        assert code == UNS and _untouched(buf), n
    assert _fill(*ok, n=_native.MAX_SAMPLES)[0] == OK and _fill(*ok, n=1)[0] == OK
    # nothing to write: no pointer is looked at
    code, buf = _fill(*ok, n_problems=0, rows=2, null=("alpha", "delta", "epsilon", "table"))
    assert code == OK and _untouched(buf)


# ---- the launch entry's host checks ----------------------------------------------------------------
def _call(lib, **kw):
    """The entry with host values that pass every check unless ``kw`` says otherwise (the device
    pointers are the address 64: a launch would follow, so every case here must return first)."""
    a = dict(nominal_path=64, BO=6, P=9, nom_so=18, nom_st=2, T=4, u0=0, count=24, n=100, l00=0.1,
             l10=0.0, l11=0.1, seed=1, state=64, zero_first=1, ego_path=64, ego_st=2, O=3, table=64,
             D=2, out=64, status=64)
    a.update(kw)
    vp = ctypes.c_void_p
    return lib.drcvar_sampled_halfspaces_f64_risk(
        vp(a["nominal_path"]), a["BO"], a["P"], a["nom_so"], a["nom_st"], a["T"], a["u0"], a["count"],
        a["n"], a["l00"], a["l10"], a["l11"], a["seed"], vp(a["state"]), a["zero_first"],
        vp(a["ego_path"]), a["ego_st"], a["O"], vp(a["table"]), a["D"], vp(a["out"]), vp(a["status"]),
        None)


def test_host_validation():
    lib = _native.risk_lib()
    assert _call(lib, count=0) == OK                       # nothing to launch ...
    assert _call(lib, count=0, **{name: None for name in POINTERS}) == OK   # ... no pointer looked at
    assert _call(lib, n=0) == OK
    nan = float("nan")
    invalid = [dict(O=0), dict(O=-2), dict(D=0), dict(D=-1),
               dict(O=4),                                   # 6 obstacle paths are not whole problems
               # a unit window outside [0, B O T)
               dict(u0=-1), dict(count=-1), dict(u0=25, count=0), dict(u0=1), dict(count=25),
               dict(u0=23, count=2),
               # what the device-state entry rejects for the shared arguments
               dict(BO=-6), dict(T=-1), dict(n=-1), dict(P=0), dict(P=-3), dict(l00=nan), dict(l10=nan),
               dict(l11=nan)]
    for kw in invalid:
        assert _call(lib, **kw) == INV, kw
    for null in POINTERS:
        assert _call(lib, **{null: None}) == INV, null
    assert _call(lib, status=None, count=0) == OK           # (status is optional)
    for off in (1, 4, 8, 12):
        assert _call(lib, state=64 + off) == INV, off
        assert _call(lib, table=64 + off) == INV, off
    assert _call(lib, table=64 + 5, count=0) == OK          # (nothing launched: the table is not read)
    # the shared limits
    assert _call(lib, n=_native.MAX_SAMPLES + 1) == UNS
    assert _call(lib, BO=3 * 2 ** 40, T=1, count=1) == UNS
    # an invalid call stays invalid whatever else it asks for
    assert _call(lib, n=_native.MAX_SAMPLES + 1, D=0) == INV
    assert _call(lib, count=0, O=0) == INV and _call(lib, count=0, D=0) == INV
    # any draw period of at least 1 passes the host, beyond B too
    for D in (1, 2, 3, 2 ** 40):
        assert _call(lib, D=D, count=0) == OK


# ---- engine.RiskTable ------------------------------------------------------------------------------
def test_risk_table_broadcasts_and_validates():
    t = RiskTable(alpha=[0.1, 0.2, 0.3], delta=0.05, epsilon=(0.0, 0.1, 0.2))
    t.validate()
    assert len(t) == 3
    assert t.row(1) == RiskParams(0.3, 0.3, 0.2, 0.05, 0.1)
    assert t.row(2) == RiskParams(0.3, 0.3, 0.3, 0.05, 0.2)
    one = RiskTable(alpha=0.2, delta=0.1, epsilon=0.15, robot_radius=0.25, obstacle_radius=0.5)
    one.validate()
    assert len(one) == 1 and one.row(0) == RiskParams(0.25, 0.5, 0.2, 0.1, 0.15)
    assert len(RiskTable(epsilon=np.linspace(0.0, 0.3, 7))) == 7
    # legal rows: alpha > 1, epsilon < 0, delta of either sign
    RiskTable(alpha=[1.5, 1.0], delta=[-0.1, 0.1], epsilon=[-0.1, 0.0]).validate()
    nan = float("nan")
    bad = [dict(alpha=[0.2, 0.0]), dict(alpha=-0.1), dict(alpha=[0.2, nan]), dict(delta=float("inf")),
           dict(epsilon=[0.1, nan]), dict(robot_radius=nan), dict(obstacle_radius=float("inf")),
           dict(alpha=[0.1, 0.2], epsilon=[0.1, 0.2, 0.3]), dict(alpha=[[0.1, 0.2]]), dict(alpha=[])]
    for kw in bad:
        with pytest.raises(ValueError):
            RiskTable(**kw).validate()
    # the filled table on the host's own "device": the rows of drcvar_risk_table_fill
    table = t.to_device(100, "cpu")
    code, buf = _fill([0.1, 0.2, 0.3], [0.05] * 3, [0.0, 0.1, 0.2], n=100)
    assert code == OK and table.dtype == torch.uint8
    assert table.numpy().tobytes() == buf[1:4].tobytes()
    with pytest.raises(_native.EngineError):
        t.to_device(_native.MAX_SAMPLES + 1, "cpu")


def _model(horizon=4):
    dt = 0.2
    A = np.array([[1, 0, dt, 0], [0, 1, 0, dt], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    B = np.array([[0.5 * dt * dt, 0], [0, 0.5 * dt * dt], [dt, 0], [0, dt]], dtype=np.float64)
    C = np.array([[1, 0, 0, 0], [0, 1, 0, 0]], dtype=np.float64)
    return MPCModel(A, B, C, np.eye(4), 0.1 * np.eye(2), horizon, device="cpu")


def test_constructors_reject_bad_risk_arguments_before_the_device():
    m = _model()
    f64 = torch.float64
    nominal, x_ref, u_ref = torch.zeros((3, 2, 9, 2), dtype=f64), torch.zeros((9, 4), dtype=f64), \
        torch.zeros((9, 2), dtype=f64)
    table = RiskTable(epsilon=[0.0, 0.1, 0.2])

    def batch(params, **kw):
        return closed_loop.RecedingHorizonBatch(m, nominal, x_ref, u_ref, 100, params, n_problems=3, **kw)

    with pytest.raises(ValueError, match="rows"):                      # the wrong length
        batch(RiskTable(epsilon=[0.0, 0.1]))
    with pytest.raises(ValueError, match="rows"):
        batch(RiskTable())
    with pytest.raises(ValueError, match="predicted"):
        batch(table, linearize="predicted")
    with pytest.raises(ValueError, match="draw_period"):               # only with a table
        batch(RiskParams(), draw_period=1)
    with pytest.raises(ValueError, match="draw_period"):
        batch(RiskParams(), draw_period=3)
    for D in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="draw_period"):
            batch(table, draw_period=D)
    with pytest.raises(ValueError, match="alpha"):
        batch(RiskTable(alpha=[0.2, 0.0, 0.2]))
    with pytest.raises(ValueError, match="RiskTable"):                 # the single-loop class
        closed_loop.RecedingHorizonFilter(m, nominal[0], x_ref, u_ref, 100, table)
    with pytest.raises(ValueError, match="RiskTable"):
        closed_loop.RecedingHorizonFilter(m, nominal[0], x_ref, u_ref, 100, RiskTable())
    # the check itself: the draw period a table gets
    assert closed_loop.check_risk(table, None, 3, "reference") == 3
    assert closed_loop.check_risk(table, 1, 3, "reference") == 1
    assert closed_loop.check_risk(table, 7, 3, "reference") == 7
    assert closed_loop.check_risk(RiskParams(), None, 3, "predicted") is None
