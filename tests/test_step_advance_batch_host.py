"""CPU: the host side of drcvar_mpc_step_advance_batch_f64 and of RecedingHorizonBatch's Python
surface.  Every call here returns or raises before any launch: no pointer is device memory and no
device is reached."""
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
POINTERS = ("x_out", "u_out", "info", "x_ref_path", "u_ref_path", "x_log", "u_log", "info_log",
            "x0", "x_ref_win", "u_fallback", "last_u", "have_last", "state")


def _model(horizon=4):
    dt = 0.2
    A = np.array([[1, 0, dt, 0], [0, 1, 0, dt], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float64)
    B = np.array([[0.5 * dt * dt, 0], [0, 0.5 * dt * dt], [dt, 0], [0, dt]], dtype=np.float64)
    C = np.array([[1, 0, 0, 0], [0, 1, 0, 0]], dtype=np.float64)
    return MPCModel(A, B, C, np.eye(4), 0.1 * np.eye(2), horizon, device="cpu")


def _advance(lib, mdl, **kw):
    a = {name: 64 for name in POINTERS}
    a.update(model=ctypes.byref(mdl), B=3, P=9, disturbance=None, step_begin=0, log_rows=5)
    a.update(kw)
    vp = ctypes.c_void_p
    return lib.drcvar_mpc_step_advance_batch_f64(
        a["model"], a["B"], vp(a["x_out"]), vp(a["u_out"]), vp(a["info"]), vp(a["x_ref_path"]),
        vp(a["u_ref_path"]), a["P"], vp(a["disturbance"]), a["step_begin"], a["log_rows"],
        vp(a["x_log"]), vp(a["u_log"]), vp(a["info_log"]), vp(a["x0"]), vp(a["x_ref_win"]),
        vp(a["u_fallback"]), vp(a["last_u"]), vp(a["have_last"]), vp(a["state"]), None)


def test_loop_library_exports_what_its_header_declares():
    """include/drcvar_loop.h, the binding and the library agree, as tests/test_abi.py holds the
    engine library to its four headers; the library holds gfx950 code."""
    text = re.sub(r"/\*.*?\*/", "", open(_native.LOOP_HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(drcvar_\w+)\s*\(", text, flags=re.M)))
    assert declared == sorted(_native.LOOP_SYMBOLS) == ["drcvar_mpc_step_advance_batch_f64"]
    assert not set(declared) & set(_native.EXPORTED_SYMBOLS)
    lib = _native.loop_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LOOP_LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert set(re.findall(r"\bT (drcvar_\w+)", out)) == set(declared)
    assert b"gfx950" in open(_native.LOOP_LIB_PATH, "rb").read()
    single = _native.lib().drcvar_mpc_step_advance_f64.argtypes
    batch = lib.drcvar_mpc_step_advance_batch_f64.argtypes
    assert batch == single[:1] + [ctypes.c_int64] + single[1:]   # n_problems after the model


def test_batch_advance_host_validation():
    lib = _native.loop_lib()
    m = _model().model
    # the single entry's checks, at any positive problem count
    for B in (1, 3, 2 ** 31 - 1):
        assert _advance(lib, m, B=B, model=None) == INV
        for null in POINTERS:
            assert _advance(lib, m, B=B, **{null: None}) == INV, null
        for off in (1, 4, 8, 12):
            assert _advance(lib, m, B=B, state=64 + off) == INV, off
        assert _advance(lib, m, B=B, log_rows=-1) == INV
        assert _advance(lib, m, B=B, P=0) == INV and _advance(lib, m, B=B, P=-1) == INV
        for field, bad in (("horizon", 0), ("horizon", _native.MPC_MAX_HORIZON + 1), ("n_states", 0),
                           ("n_states", _native.MPC_MAX_STATES + 1), ("n_inputs", 0),
                           ("n_inputs", _native.MPC_MAX_INPUTS + 1)):
            broken = _native.MpcModel.from_buffer_copy(m)
            setattr(broken, field, bad)
            assert _advance(lib, broken, B=B) == INV, (field, bad)
    # the problem count
    assert _advance(lib, m, B=-1) == INV and _advance(lib, m, B=-2 ** 63) == INV
    for B in (2 ** 31, 2 ** 40, 2 ** 63 - 1):
        assert _advance(lib, m, B=B) == UNS, B
        assert _advance(lib, m, B=B, state=None) == INV   # an invalid call stays invalid
    # nothing to do: no launch, no other argument is looked at
    assert _advance(lib, m, B=0) == OK
    assert _advance(lib, m, B=0, model=None, **{name: None for name in POINTERS}) == OK


def _paths(B=3, O=2, P=9):
    f64 = torch.float64
    return (torch.zeros((B, O, P, 2), dtype=f64), torch.zeros((P, 4), dtype=f64),
            torch.zeros((P, 2), dtype=f64))


def test_batch_shape_checks():
    nominal, _, _ = _paths()
    f64 = torch.float64
    check = closed_loop.check_batch_shapes
    assert check(nominal, None, 3, 4) == (2, 9)
    assert check(nominal[0], None, 3, 4) == (2, 9)             # one scenario for every problem
    assert check(nominal, torch.zeros((3, 5, 4), dtype=f64), 3, 4) == (2, 9)
    for B in (2, 4):                                            # nominal_path against n_problems
        with pytest.raises(ValueError, match="n_problems"):
            check(nominal, None, B, 4)
    for B in (0, -1):
        with pytest.raises(ValueError, match="n_problems"):
            check(nominal, None, B, 4)
    for bad in (nominal.float(), torch.zeros((3, 2, 9, 3), dtype=f64), torch.zeros((9, 2), dtype=f64),
                torch.zeros((3, 0, 9, 2), dtype=f64), torch.zeros((3, 2, 0, 2), dtype=f64), None):
        with pytest.raises(ValueError):
            check(bad, None, 3, 4)
    for rows in (2, 4):                                         # disturbance against n_problems
        with pytest.raises(ValueError, match="n_problems"):
            check(nominal, torch.zeros((rows, 5, 4), dtype=f64), 3, 4)
    for bad in (torch.zeros((5, 4), dtype=f64), torch.zeros((3, 5, 3), dtype=f64),
                torch.zeros((3, 0, 4), dtype=f64), torch.zeros((3, 5, 4), dtype=torch.float32)):
        with pytest.raises(ValueError):
            check(nominal, bad, 3, 4)


def test_batch_x0_shapes():
    x0 = closed_loop.batch_x0(np.arange(4.0), 3, 4)
    assert tuple(x0.shape) == (3, 4) and x0.dtype == torch.float64
    assert torch.equal(x0, torch.arange(4.0, dtype=torch.float64).expand(3, 4))
    per = np.arange(12.0).reshape(3, 4)
    assert torch.equal(closed_loop.batch_x0(per, 3, 4), torch.from_numpy(per))
    for bad, B in ((per, 2), (per, 4), (np.zeros(3), 3), (np.zeros((3, 5)), 3), (np.zeros((1, 4)), 3),
                   (np.zeros(12), 3)):
        with pytest.raises(ValueError):
            closed_loop.batch_x0(bad, B, 4)


def test_batch_constructor_rejects_before_the_device():
    m = _model()
    nominal, x_ref, u_ref = _paths()
    p = RiskParams()
    f64 = torch.float64
    make = closed_loop.RecedingHorizonBatch
    with pytest.raises(TypeError):                              # n_problems is required
        make(m, nominal, x_ref, u_ref, 100, p)
    mismatched = [
        dict(n_problems=2), dict(n_problems=4), dict(n_problems=0),
        dict(disturbance=torch.zeros((2, 5, 4), dtype=f64)),
        dict(disturbance=torch.zeros((5, 4), dtype=f64)),
    ]
    for kw in mismatched:
        a = dict(n_problems=3)
        a.update(kw)
        with pytest.raises(ValueError, match="n_problems|disturbance must be"):
            make(m, nominal, x_ref, u_ref, 100, p, **a)
    others = [
        dict(nominal_path=nominal.float()), dict(nominal_path=torch.zeros((3, 2, 9), dtype=f64)),
        dict(x_ref_path=torch.zeros((8, 4), dtype=f64)), dict(x_ref_path=torch.zeros((9, 3), dtype=f64)),
        dict(u_ref_path=torch.zeros((10, 2), dtype=f64)), dict(u_ref_path=u_ref.float()),
        dict(),                                                 # every path on the host
    ]
    for kw in others:
        a = dict(nominal_path=nominal, x_ref_path=x_ref, u_ref_path=u_ref)
        a.update(kw)
        with pytest.raises(ValueError):
            make(m, a["nominal_path"], a["x_ref_path"], a["u_ref_path"], 100, p, n_problems=3)
    for kw in (dict(metric="median"), dict(steps_per_graph=0)):
        with pytest.raises(ValueError):
            make(m, nominal, x_ref, u_ref, 100, p, n_problems=3, **kw)
    with pytest.raises(ValueError):
        make(m, nominal, x_ref, u_ref, _native.MAX_SAMPLES + 1, p, n_problems=3)


def test_batch_run_argument_checks():
    """run()'s checks are the single class's (check_run_steps): a bad backend and steps that do not
    fill whole graphs are rejected before the loop is looked at."""
    loop = closed_loop.RecedingHorizonBatch.__new__(closed_loop.RecedingHorizonBatch)
    loop.steps_per_graph = 3
    for n, backend in ((4, "graph"), (3, "eager"), (-3, "launches")):
        with pytest.raises(ValueError):
            loop.run(n, backend=backend)
