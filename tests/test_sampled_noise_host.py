"""CPU: the host side of the noise library (include/drcvar_loop_noise.h): the symbol lists, the
host checks of drcvar_sampled_halfspaces_f64_noise, drcvar_noise_table_fill and engine.NoiseTable.
Every call here returns or raises before any launch: no pointer is device memory and no device is
reached."""
import ctypes
import math
import re
import struct
import subprocess

import numpy as np
import pytest

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import NoiseTable

INV, UNS, OK = _native.ERR_INVALID_ARGUMENT, _native.ERR_UNSUPPORTED, _native.OK
POINTERS = ("nominal_path", "state", "ego_path", "table", "metric", "out", "selected")


def _symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return set(re.findall(r"\bT (drcvar_\w+)", out))


def test_noise_library_exports_what_its_header_declares():
    text = re.sub(r"/\*.*?\*/", "", open(_native.NOISE_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(drcvar_\w+)\s*\(", text, flags=re.M)))
    assert declared == sorted(_native.NOISE_SYMBOLS)
    assert declared == ["drcvar_noise_table_fill", "drcvar_noise_table_row_bytes",
                        "drcvar_sampled_halfspaces_f64_noise"]
    lib = _native.noise_lib()
    assert _symbols(_native.NOISE_LIB_PATH) == set(declared)
    assert b"gfx950" in open(_native.NOISE_LIB_PATH, "rb").read()
    # the other seven lists are what they were, and disjoint from the new one
    lists = (_native.EXPORTED_SYMBOLS, _native.LOOP_SYMBOLS, _native.EVAL_SYMBOLS, _native.PRED_SYMBOLS,
             _native.RISK_SYMBOLS, _native.METRIC_SYMBOLS, _native.ROUTE_SYMBOLS)
    for other in lists:
        assert not set(declared) & set(other)
    for path, symbols in zip((_native.LIB_PATH, _native.LOOP_LIB_PATH, _native.EVAL_LIB_PATH,
                              _native.PRED_LIB_PATH, _native.RISK_LIB_PATH, _native.METRIC_LIB_PATH,
                              _native.ROUTE_LIB_PATH), lists):
        assert _symbols(path) == set(symbols), path
    assert tuple(len(s) for s in lists) == (33, 1, 2, 1, 3, 2, 2)
    assert _native.ABI_VERSION == 3
    src, defs = _native.NOISE_UNIT
    assert src in _native.SOURCES and src.endswith("drcvar_sampled.hip")
    assert defs == ("-DDRCVAR_LOOP_NOISE_LIBRARY",)
    # the route entry's argument list with the three doubles replaced by a pointer and a period
    noise = lib.drcvar_sampled_halfspaces_f64_noise.argtypes
    route = _native.route_lib().drcvar_sampled_halfspaces_f64_route.argtypes
    assert len(noise) == 25 and noise == route[:9] + [ctypes.c_void_p, ctypes.c_int64] + route[12:]


# ---- the entry's host checks -------------------------------------------------------------------------
def _call(lib, entry="noise", **kw):
    """The entry with host values that pass every check unless ``kw`` says otherwise (the device
    pointers are the address 64: a launch would follow, so every case here must return first).
    ``entry="route"``: the same arguments, with a factor in place of the table, to the route entry."""
    a = dict(nominal_path=64, BO=6, P=9, nom_so=18, nom_st=2, T=4, u0=0, count=24, n=100, noise=64,
             NP=3, seed=1, state=64, zero_first=1, ego_path=64, ego_st=2, ego_ps=18, O=3,
             table=64, D=2, metric=64, out=64, status=64, selected=64)
    a.update(kw)
    vp = ctypes.c_void_p
    head = (vp(a["nominal_path"]), a["BO"], a["P"], a["nom_so"], a["nom_st"], a["T"], a["u0"], a["count"],
            a["n"])
    tail = (a["seed"], vp(a["state"]), a["zero_first"], vp(a["ego_path"]), a["ego_st"], a["ego_ps"],
            a["O"], vp(a["table"]), a["D"], vp(a["metric"]), vp(a["out"]), vp(a["status"]),
            vp(a["selected"]), None)
    if entry == "route":
        return lib.drcvar_sampled_halfspaces_f64_route(*head, 0.1, 0.0, 0.1, *tail)
    return lib.drcvar_sampled_halfspaces_f64_noise(*head, vp(a["noise"]), a["NP"], *tail)


def test_noise_halfspace_host_validation():
    lib, route = _native.noise_lib(), _native.route_lib()
    assert _call(lib, count=0) == OK                       # nothing to launch ...
    assert _call(lib, count=0, noise=None, **{name: None for name in POINTERS}) == OK   # ... no pointer
    assert _call(lib, n=0) == OK and _call(lib, n=0, noise=None) == OK
    # everything the route entry rejects, with its code, at several periods
    rejected = [dict(ego_ps=-1), dict(ego_ps=2 ** 40 + 1), dict(O=0), dict(O=-2), dict(D=0), dict(D=-1),
                dict(O=4), dict(u0=-1), dict(count=-1), dict(u0=25, count=0), dict(u0=1), dict(count=25),
                dict(u0=23, count=2), dict(T=-1), dict(n=-1), dict(P=0), dict(P=-3),
                dict(n=_native.MAX_SAMPLES + 1), dict(BO=3 * 2 ** 40, T=1, count=1),
                dict(n=_native.MAX_SAMPLES + 1, D=0), dict(count=0, O=0), dict(count=0, D=0)]
    rejected += [{name: None} for name in POINTERS]
    rejected += [dict(state=64 + off) for off in (1, 4, 8, 12)] + [dict(table=64 + off) for off in (1, 4, 8, 12)]
    for kw in rejected:
        want = _call(route, "route", **kw)
        assert want in (INV, UNS), kw
        for period in (1, 3, 6):
            assert _call(lib, NP=period, **kw) == want, (kw, period)
    assert sum(_call(route, "route", **kw) == UNS for kw in rejected) == 3
    # the period of its own: before everything else (an unsupported call with a bad period is invalid)
    for period in (0, -1, 7, 2 ** 40, -2 ** 63):
        assert _call(lib, NP=period) == INV, period
        assert _call(lib, NP=period, count=0) == INV, period
        assert _call(lib, NP=period, ego_ps=2 ** 40 + 1) == INV, period
    assert _call(lib, BO=-6) == INV
    for period in (1, 3, 6):
        assert _call(lib, NP=period, count=0) == OK
    # the table's pointer: once there is something to launch, and before the route entry's checks
    for bad in (None, 65, 68, 72, 76):
        assert _call(lib, noise=bad) == INV, bad
        assert _call(lib, noise=bad, ego_ps=2 ** 40 + 1) == INV, bad
        assert _call(lib, noise=bad, count=0) == OK, bad
        assert _call(lib, noise=bad, n=0) == OK, bad
    assert _call(lib, status=None, count=0) == OK           # (status is optional)


# ---- the table's fill ----------------------------------------------------------------------------------
def _fill(chol, out_bytes=None, rows=None):
    lib = _native.noise_lib()
    c = np.ascontiguousarray(np.asarray(chol, dtype=np.float64).reshape(-1, 3))
    n = c.shape[0] if rows is None else rows
    row = int(lib.drcvar_noise_table_row_bytes())
    host = np.full((max(c.shape[0], 1), row), 0xAB, dtype=np.uint8)
    code = lib.drcvar_noise_table_fill(c.ctypes.data, n, host.ctypes.data,
                                       host.nbytes if out_bytes is None else out_bytes)
    return code, host


def _row(host, r=0):
    """(l00, l10, l11, iso, lam) of row r: the three doubles, the flag word and the log scale's lam."""
    l00, l10, l11, iso, lam = struct.unpack_from("<dddqd", host[r].tobytes())
    return l00, l10, l11, iso, lam


def test_noise_table_fill():
    lib = _native.noise_lib()
    row = int(lib.drcvar_noise_table_row_bytes())
    assert row > 0 and row % 16 == 0
    up = lambda v: math.nextafter(v, math.inf)
    down = lambda v: math.nextafter(v, 0.0)
    lo = 2.0 ** -100                      # l00^2 = 2^-200 exactly
    inf = float("inf")
    cases = [((0.1, 0.0, 0.1), True), ((0.1, 0.0, up(0.1)), False), ((up(0.1), 0.0, 0.1), False),
             ((0.1, -0.0, 0.1), True), ((0.1, 5e-324, 0.1), False), ((0.0, 0.0, 0.0), False),
             ((-0.1, 0.0, -0.1), False), ((lo, 0.0, lo), True), ((down(lo), 0.0, down(lo)), False),
             ((2.0 ** 100, 0.0, 2.0 ** 100), True), ((up(2.0 ** 100), 0.0, up(2.0 ** 100)), False),
             ((inf, 0.0, inf), False), ((1.0, 0.0, 0.0), False), ((0.1, 0.05, 0.2), False)]
    code, host = _fill([c for c, _ in cases])
    assert code == OK
    for r, (chol, iso) in enumerate(cases):
        l00, l10, l11, flag, lam = _row(host, r)
        got = struct.pack("<ddd", l00, l10, l11)
        assert got == struct.pack("<ddd", *chol), chol       # the factor's bits, -0.0 included
        assert flag == (1 if iso else 0), chol
        assert lam == (chol[0] * chol[0] if iso else 1.0), chol
    # equal factors give equal bytes, nothing of the fill pattern is left
    code, twice = _fill([cases[0][0], cases[0][0]])
    assert code == OK and twice[0].tobytes() == twice[1].tobytes() == host[0].tobytes()
    # NaN anywhere: rejected, and nothing written
    nan = float("nan")
    for k in range(3):
        chol = [[0.1, 0.0, 0.1], [0.2, 0.0, 0.2]]
        chol[1][k] = nan
        code, host = _fill(chol)
        assert code == INV and np.all(host == 0xAB), k
    # a short buffer, bad counts, null pointers
    code, host = _fill([[0.1, 0.0, 0.1]] * 2, out_bytes=2 * row - 1)
    assert code == INV and np.all(host == 0xAB)
    assert _fill([[0.1, 0.0, 0.1]] * 2, out_bytes=2 * row)[0] == OK
    assert _fill([[0.1, 0.0, 0.1]], rows=-1)[0] == INV
    assert _fill([[0.1, 0.0, 0.1]], out_bytes=-1)[0] == INV
    assert lib.drcvar_noise_table_fill(None, 0, None, 0) == OK
    buf = np.zeros(row, dtype=np.uint8)
    one = np.array([0.1, 0.0, 0.1])
    assert lib.drcvar_noise_table_fill(None, 1, buf.ctypes.data, row) == INV
    assert lib.drcvar_noise_table_fill(one.ctypes.data, 1, None, row) == INV


# ---- NoiseTable --------------------------------------------------------------------------------------
def test_noise_table_shapes_and_period():
    H, O, B = 4, 2, 3
    one = NoiseTable(np.full((H, 3), 0.1))
    per_obstacle = NoiseTable(np.full((O, H, 3), 0.1))
    per_problem = NoiseTable(np.full((B, O, H, 3), 0.1))
    assert (one.period(B, O), per_obstacle.period(B, O), per_problem.period(B, O)) == (1, O, B * O)
    assert one.horizon == per_obstacle.horizon == per_problem.horizon == H
    with pytest.raises(ValueError, match="leading dimensions"):
        per_obstacle.period(B, O + 1)
    with pytest.raises(ValueError, match="leading dimensions"):
        per_problem.period(B + 1, O)
    for bad in (np.zeros(3), np.zeros((H, 2)), np.zeros((0, 3)), np.zeros((1, 2, 3, 4, 3))):
        with pytest.raises(ValueError, match="shape"):
            NoiseTable(bad).validate()
    with pytest.raises(ValueError, match="NaN"):
        NoiseTable(np.full((H, 3), float("nan"))).validate()
    NoiseTable(np.array([[0.0, 0.0, 0.0], [float("inf"), 0.0, 1.0]])).validate()
    chol = np.arange(B * O * H * 3, dtype=np.float64).reshape(B, O, H, 3)
    table = NoiseTable(chol)
    for o in range(B * O):
        for t in range(H):
            assert table.factor(o, t) == tuple(chol.reshape(B * O, H, 3)[o, t])
    assert NoiseTable(chol[0]).factor(O + 1, 2) == tuple(chol[0, 1, 2])      # o mod period
    assert NoiseTable(chol[0, 0]).factor(5, 3) == tuple(chol[0, 0, 3])
    host = table.to_device("cpu")
    row = int(_native.noise_lib().drcvar_noise_table_row_bytes())
    assert tuple(host.shape) == (B * O * H, row)
    assert _row(host.numpy(), 7)[:3] == tuple(chol.reshape(-1, 3)[7])


def test_scaled_by_one_is_the_noise_factor_bit_for_bit():
    H = 5
    for cov in (engine.DEFAULT_NOISE_COV, ((0.04, 0.01), (0.01, 0.09))):
        want = struct.pack("<ddd", *engine._noise_factor(cov, None))
        table = NoiseTable.scaled(cov, np.ones(H))
        for t in range(H):
            assert struct.pack("<ddd", *table.factor(0, t)) == want
        assert NoiseTable.from_cov(np.broadcast_to(np.array(cov), (H, 2, 2))).factor(0, H - 1) == \
            table.factor(0, 0)
    grown = NoiseTable.scaled(engine.DEFAULT_NOISE_COV, 1.0 + 0.5 * np.arange(H))
    for t in range(H):
        cov = (1.0 + 0.5 * t) * np.array(engine.DEFAULT_NOISE_COV)
        assert grown.factor(0, t) == engine._noise_factor(cov, None)
    per_problem = NoiseTable.scaled(engine.DEFAULT_NOISE_COV, np.ones((3, 2, H)))
    assert per_problem.period(3, 2) == 6 and per_problem.horizon == H


# ---- RecedingHorizonBatch(noise=...) -------------------------------------------------------------------
def _model(horizon=4):
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core.mpc_filter import MPCModel
    dt = 0.2
    A = np.array([[1, 0, dt, 0], [0, 1, 0, dt], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    Bm = np.array([[0.5 * dt * dt, 0], [0, 0.5 * dt * dt], [dt, 0], [0, dt]], dtype=np.float64)
    C = np.array([[1, 0, 0, 0], [0, 1, 0, 0]], dtype=np.float64)
    return MPCModel(A, Bm, C, np.eye(4), 0.1 * np.eye(2), horizon, device="cpu")


def test_batch_noise_argument_errors_need_no_device():
    import torch
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.closed_loop import (
        RecedingHorizonBatch)
    H, O, P, B = 4, 2, 9, 3
    model = _model(H)
    nominal = torch.zeros((O, P, 2), dtype=torch.float64)
    x_ref, u_ref = torch.zeros((P, 4), dtype=torch.float64), torch.zeros((P, 2), dtype=torch.float64)
    good = NoiseTable(np.full((O, H, 3), 0.1))

    def build(noise, **kw):
        return RecedingHorizonBatch(model, nominal, x_ref, u_ref, 20, RiskParams(), n_problems=B,
                                    noise=noise, **kw)
    with pytest.raises(ValueError, match="NoiseTable"):
        build(np.full((H, 3), 0.1))
    with pytest.raises(ValueError, match="predicted"):
        build(good, linearize="predicted")
    with pytest.raises(ValueError, match="defaults"):
        build(good, chol=(0.1, 0.0, 0.1))
    with pytest.raises(ValueError, match="defaults"):
        build(good, noise_cov=[[0.02, 0.0], [0.0, 0.02]])
    with pytest.raises(ValueError, match="NaN"):
        build(NoiseTable(np.full((H, 3), float("nan"))))
    with pytest.raises(ValueError, match="horizon"):
        build(NoiseTable(np.full((H + 1, 3), 0.1)))
    with pytest.raises(ValueError, match="leading dimensions"):
        build(NoiseTable(np.full((O + 1, H, 3), 0.1)))
    with pytest.raises(ValueError, match="leading dimensions"):
        build(NoiseTable(np.full((B + 1, O, H, 3), 0.1)))
