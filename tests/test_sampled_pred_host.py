"""CPU: the host side of drcvar_sampled_halfspaces_f64_pred (include/drcvar_loop_pred.h) and of the
linearize= / relinearize= surface of the loop classes.  Every call here returns or raises before
any launch: no pointer is device memory and no device is reached."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core.mpc_filter import MPCModel
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import closed_loop

INV, UNS, OK = _native.ERR_INVALID_ARGUMENT, _native.ERR_UNSUPPORTED, _native.OK
POINTERS = ("nominal_path", "state", "x0", "pred", "c_out", "out")
C_OUT = (ctypes.c_double * 16)(*([0.0] * 16))


def _call(lib, **kw):
    """The entry with host values that pass every check unless ``kw`` says otherwise (the device
    pointers are the address 64: a launch would follow, so every case here must return first)."""
    a = dict(nominal_path=64, BO=6, P=9, nom_so=18, nom_st=2, T=4, u0=0, count=24, n=100, l00=0.1,
             l10=0.0, l11=0.1, seed=1, state=64, zero_first=1, O=3, x0=64, pred=64, rows=5, nx=4,
             c_out=ctypes.addressof(C_OUT), shift=1, rr=0.3, ro=0.3, alpha=0.2, delta=0.1, eps=0.15,
             out=64, status=64)
    a.update(kw)
    vp = ctypes.c_void_p
    return lib.drcvar_sampled_halfspaces_f64_pred(
        vp(a["nominal_path"]), a["BO"], a["P"], a["nom_so"], a["nom_st"], a["T"], a["u0"], a["count"],
        a["n"], a["l00"], a["l10"], a["l11"], a["seed"], vp(a["state"]), a["zero_first"], a["O"],
        vp(a["x0"]), vp(a["pred"]), a["rows"], a["nx"], vp(a["c_out"]), a["shift"], a["rr"], a["ro"],
        a["alpha"], a["delta"], a["eps"], vp(a["out"]), vp(a["status"]), None)


def _symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return set(re.findall(r"\bT (drcvar_\w+)", out))


def test_pred_library_exports_what_its_header_declares():
    text = re.sub(r"/\*.*?\*/", "", open(_native.PRED_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(drcvar_\w+)\s*\(", text, flags=re.M)))
    assert declared == sorted(_native.PRED_SYMBOLS)
    assert declared == ["drcvar_sampled_halfspaces_f64_pred"]
    others = set(_native.EXPORTED_SYMBOLS) | set(_native.LOOP_SYMBOLS) | set(_native.EVAL_SYMBOLS)
    assert not set(declared) & others
    lib = _native.pred_lib()
    assert _symbols(_native.PRED_LIB_PATH) == set(declared)
    assert b"gfx950" in open(_native.PRED_LIB_PATH, "rb").read()
    assert len(lib.drcvar_sampled_halfspaces_f64_pred.argtypes) == 30
    # the other three libraries export what they did
    for path, symbols in ((_native.LIB_PATH, _native.EXPORTED_SYMBOLS),
                          (_native.LOOP_LIB_PATH, _native.LOOP_SYMBOLS),
                          (_native.EVAL_LIB_PATH, _native.EVAL_SYMBOLS)):
        assert _symbols(path) == set(symbols), path
    assert (len(_native.EXPORTED_SYMBOLS), len(_native.LOOP_SYMBOLS), len(_native.EVAL_SYMBOLS)) == (33, 1, 2)
    assert _native.ABI_VERSION == 3
    # the same source, compiled once more with a define of its own
    src, defs = _native.PRED_UNIT
    assert src in _native.SOURCES and src.endswith("drcvar_sampled.hip")
    assert defs == ("-DDRCVAR_LOOP_PRED_LIBRARY",)


def test_host_validation():
    lib = _native.pred_lib()
    assert _call(lib, count=0) == OK                       # nothing to launch ...
    assert _call(lib, count=0, **{name: None for name in POINTERS}) == OK   # ... no pointer looked at
    assert _call(lib, n=0) == OK
    nan = float("nan")
    invalid = [dict(nx=0), dict(nx=9), dict(nx=-1), dict(O=0), dict(O=-2), dict(rows=0), dict(rows=-1),
               dict(shift=2), dict(shift=-1),
               dict(O=4),                                   # 6 obstacle paths are not whole problems
               # a unit window outside [0, B O T)
               dict(u0=-1), dict(count=-1), dict(u0=25, count=0), dict(u0=1), dict(count=25),
               dict(u0=23, count=2),
               # what the device-state entry rejects for the shared arguments
               dict(BO=-6), dict(T=-1), dict(n=-1), dict(P=0), dict(P=-3), dict(l00=nan), dict(l10=nan),
               dict(l11=nan), dict(rr=nan), dict(ro=float("inf")), dict(alpha=0.0), dict(alpha=nan)]
    for kw in invalid:
        assert _call(lib, **kw) == INV, kw
    for null in POINTERS:
        assert _call(lib, **{null: None}) == INV, null
    assert _call(lib, status=None, count=0) == OK           # (status is optional)
    for off in (1, 4, 8, 12):
        assert _call(lib, state=64 + off) == INV, off
    # the shared limits
    assert _call(lib, n=_native.MAX_SAMPLES + 1) == UNS
    assert _call(lib, BO=3 * 2 ** 40, T=1, count=1) == UNS
    # an invalid call stays invalid whatever else it asks for
    assert _call(lib, n=_native.MAX_SAMPLES + 1, shift=2) == INV
    assert _call(lib, count=0, nx=9) == INV and _call(lib, count=0, shift=3) == INV


def _model(horizon=4):
    dt = 0.2
    A = np.array([[1, 0, dt, 0], [0, 1, 0, dt], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    B = np.array([[0.5 * dt * dt, 0], [0, 0.5 * dt * dt], [dt, 0], [0, dt]], dtype=np.float64)
    C = np.array([[1, 0, 0, 0], [0, 1, 0, 0]], dtype=np.float64)
    return MPCModel(A, B, C, np.eye(4), 0.1 * np.eye(2), horizon, device="cpu")


def test_constructors_reject_bad_linearize_arguments_before_the_device():
    m = _model()
    f64 = torch.float64
    nominal, x_ref, u_ref = torch.zeros((3, 2, 9, 2), dtype=f64), torch.zeros((9, 4), dtype=f64), \
        torch.zeros((9, 2), dtype=f64)
    bad = [dict(linearize="actual"), dict(linearize=None), dict(linearize="predicted", relinearize=-1),
           dict(relinearize=-1), dict(relinearize=1), dict(linearize="reference", relinearize=2),
           dict(linearize="predicted", relinearize=1.5)]
    for kw in bad:
        with pytest.raises(ValueError, match="linearize"):
            closed_loop.RecedingHorizonBatch(m, nominal, x_ref, u_ref, 100, RiskParams(), n_problems=3, **kw)
        with pytest.raises(ValueError, match="linearize"):
            closed_loop.RecedingHorizonFilter(m, nominal[0], x_ref, u_ref, 100, RiskParams(), **kw)
    assert closed_loop.LINEARIZE == ("reference", "predicted")
    for ok in (dict(linearize="reference", relinearize=0), dict(linearize="predicted", relinearize=0),
               dict(linearize="predicted", relinearize=3)):
        closed_loop.check_linearize(**ok)
