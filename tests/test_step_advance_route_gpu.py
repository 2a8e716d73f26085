"""GPU: drcvar_mpc_step_advance_batch_route_f64 (csrc/drcvar_step.hip, include/drcvar_loop_route.h)
against B = 3 calls of the single entry drcvar_mpc_step_advance_f64 on each problem's slices with
that problem's own paths, and against tests/step_advance_mirror.py per problem, BIT FOR BIT: the
launch is copies plus one IEEE addition of finite numbers per state element, so there is no
tolerance in this file.

The layout, the guards and the comparison are those of tests/test_step_advance_batch_gpu.py, with
the two paths stacked per problem: ``[B, R, nx]`` and ``[B, R, nu]`` with R >= P rows, so that the
problem strides R nx and R nu are the dense ones (R = P) or larger (R = P + 2; the rows past P hold
a sentinel that no window may show).  Every problem has its own random paths, so a kernel that
reads problem 0's paths for everyone fails in problems 1 and 2.

Shapes: (10, 4, 2) and the ABI's limits (64, 8, 4): 256 threads own an input element, 520 window
elements take three passes.  Inside one launch the three problems differ in status (a solved, a
failed and a NaN one side by side), have_last, step and stream offset; the plans cross that with a
disturbance present and NULL, no log rows at all, and paths shorter than the window (P = H and
P = 1); one launch holds steps -2^63 and 2^63 - 1.  With both strides 0 the launch is compared with
the batch entry's.
"""
import ctypes

import numpy as np
import pytest
import torch

import step_advance_cases as sc
import step_advance_mirror as sm
import test_step_advance_batch_gpu as tb
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native

pytestmark = pytest.mark.gpu
B = 3
SHAPES = [(10, 4, 2), (64, 8, 4)]
PATHS = ("x_ref_path", "u_ref_path")
PATH_FILL = 4.2e+88                     # the rows between one problem's path and the next one's
STATUS_SETS = ((0.0, 1.0, sc.NAN), (3.0, 4.0, 0.5), (sc.NAN, 0.0, 2.0), (5.0, sc.NAN, 3.0))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def route_cases(H, nx, nu, P, begin, rows, disturbed, steps, shift):
    """The batch file's cycling cases for B = 3, with a status set that holds a solved, a failed
    and (in three of four) a NaN status."""
    cases = tb.batch_cases(H, nx, nu, B, P, begin, rows, disturbed, steps, shift)
    statuses = STATUS_SETS[shift % len(STATUS_SETS)]
    return [c._replace(status=statuses[b]) for b, c in enumerate(cases)]


def make_problems(cases):
    """[(buffers, state)] per problem: every problem its own paths (its own seed)."""
    return [sc.make_buffers(c) for c in cases]


def pack(problems, pad_rows):
    """`test_step_advance_batch_gpu.pack` with the paths stacked per problem to ``[B, P + pad_rows,
    .]``, the rows past P filled with PATH_FILL."""
    first = problems[0][0]
    items = []
    for name in sm.BUFFERS:
        if first[name] is None:
            continue
        if name in PATHS:
            stacked = np.stack([b[name] for b, _ in problems])
            fill = np.full((len(problems), pad_rows, stacked.shape[2]), PATH_FILL)
            items.append((name, np.concatenate([stacked, fill], axis=1)))
        elif name == "have_last":
            items.append((name, np.concatenate([b[name] for b, _ in problems]).astype(np.int32)))
        else:
            items.append((name, np.stack([b[name] for b, _ in problems])))
    items.append(("state", np.array([[s[0], s[1] % 2 ** 64] for _, s in problems], dtype=np.uint64)))
    chunks, regions, at = [], {}, 0
    for name, a in items:
        guard = (np.full(sc.GUARD_BYTES // 4, sc.GUARD_I32, dtype=np.int32) if a.dtype == np.int32
                 else np.full(sc.GUARD_BYTES // 8, sc.GUARD_F64))
        pad = guard[:(-a.nbytes % 16) // guard.itemsize]
        regions[name] = (at + sc.GUARD_BYTES, a.shape, a.dtype)
        for piece in (guard, a.reshape(-1), pad, guard):
            chunks.append(piece.view(np.uint8))
            at += piece.nbytes
        assert at % 16 == 0
    return np.concatenate(chunks), regions


def _model(c):
    model = _native.MpcModel()
    model.horizon, model.n_states, model.n_inputs, model.n_outputs = c.H, c.nx, c.nu, 2
    return model


def launch_route(cases, arena, regions, strides):
    """One route launch on the device bytes `arena`; a buffer without a region is NULL."""
    c = cases[0]
    assert arena.data_ptr() % 16 == 0 and regions["state"][0] % 16 == 0
    model = _model(c)
    at = lambda name: ctypes.c_void_p(arena.data_ptr() + regions[name][0] if name in regions else None)
    stream = torch.cuda.current_stream(arena.device).cuda_stream
    rc = _native.route_lib().drcvar_mpc_step_advance_batch_route_f64(
        ctypes.byref(model), len(cases), *(at(n) for n in tb.ARGUMENTS), c.path_steps, *strides,
        at("disturbance"), c.step_begin, c.log_rows, *(at(n) for n in tb.FIXED), ctypes.c_void_p(stream))
    assert rc == _native.OK, c
    return arena.cpu().numpy()


def launch_singles(cases, arena, regions):
    """B calls of the single entry, call b on problem b's slice of every region."""
    c = cases[0]
    model = _model(c)
    stream = torch.cuda.current_stream(arena.device).cuda_stream

    def at(name, b):
        if name not in regions:
            return ctypes.c_void_p(None)
        offset, shape, dtype = regions[name]
        per_problem = int(np.prod(shape[1:])) * np.dtype(dtype).itemsize
        return ctypes.c_void_p(arena.data_ptr() + offset + b * per_problem)

    for b in range(len(cases)):
        rc = _native.lib().drcvar_mpc_step_advance_f64(
            ctypes.byref(model), *(at(n, b) for n in tb.ARGUMENTS), c.path_steps, at("disturbance", b),
            c.step_begin, c.log_rows, *(at(n, b) for n in tb.FIXED), ctypes.c_void_p(stream))
        assert rc == _native.OK, (c, b)
    return arena.cpu().numpy()


def check_launch(dev, cases, pad_rows):
    c = cases[0]
    problems = make_problems(cases)
    for b in (1, 2):        # the paths differ from problem to problem
        assert not np.array_equal(problems[0][0]["x_ref_path"], problems[b][0]["x_ref_path"])
    pre, regions = pack(problems, pad_rows)
    rows = c.path_steps + pad_rows
    strides = (rows * c.nx, rows * c.nu)
    assert regions["x_ref_path"][1] == (B, rows, c.nx) and regions["u_ref_path"][1] == (B, rows, c.nu)
    want, _ = pack(tb.mirror(cases, problems), pad_rows)
    got = launch_route(cases, torch.from_numpy(pre).to(dev), regions, strides)
    bad = tb.mismatches(cases, got, pre, want, regions)
    assert not bad, (c, pad_rows, bad)
    singles = launch_singles(cases, torch.from_numpy(pre).to(dev), regions)
    assert got.tobytes() == singles.tobytes(), (c, pad_rows, "differs from B calls of the single entry")
    assert got.tobytes() == want.tobytes(), (c, pad_rows)


@pytest.mark.parametrize("pad_rows", [0, 2], ids=["dense", "wider-stride"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H%d-nx%d-nu%d" % s)
def test_route_advance_equals_the_single_entry_per_problem(dev, shape, pad_rows):
    """Every plan of the batch file (disturbed; P = H undisturbed; P = 1 with no log rows), four
    slices of the step / offset / have_last cycles each."""
    H, nx, nu = shape
    seen = set()
    for n, (name, P, begin, rows, disturbed, steps) in enumerate(tb.plans(H)):
        for shift in (0, 3, 6, 9):
            cases = route_cases(H, nx, nu, P, begin, rows, disturbed, steps, shift + n)
            seen.update(repr(c.status) for c in cases)
            check_launch(dev, cases, pad_rows)
    assert {repr(s) for s in (0.0, 1.0, sc.NAN)} <= seen
    assert [p[1] for p in tb.plans(H)] == [3 * H + 5, H, 1] and tb.plans(H)[2][3] == 0


def test_a_solved_a_failed_and_a_nan_status_side_by_side():
    """(needs no device) the first status set is the one the docstring names."""
    H = 10
    name, P, begin, rows, disturbed, steps = tb.plans(H)[0]
    cases = route_cases(H, 4, 2, P, begin, rows, disturbed, steps, 0)
    assert [repr(c.status) for c in cases] == [repr(s) for s in (0.0, 1.0, sc.NAN)]
    assert len({c.step for c in cases}) == 3 and len({c.offset for c in cases}) == 3


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H%d-nx%d-nu%d" % s)
def test_the_ends_of_int64_side_by_side(dev, shape):
    """Steps -2^63, 2^63 - 1 and 2^63 - 2 with step_begin = 2^63 - 1: problem 0 logs row 1 by
    wrapping, problem 1 row 0, problem 2 nothing; every window row is its own path's first / last."""
    H, nx, nu = shape
    for disturbed in (False, True):
        cases = route_cases(H, nx, nu, 3 * H + 5, sc.INT64_MAX, 3, disturbed,
                            [sc.INT64_MIN, sc.INT64_MAX, sc.INT64_MAX - 1], 0)
        assert [sc.log_index(c) for c in cases] == [(1, True), (0, True), (2 ** 64 - 1, False)]
        check_launch(dev, cases, 0)
        check_launch(dev, cases[::-1], 2)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H%d-nx%d-nu%d" % s)
def test_strides_zero_are_the_batch_entry(dev, shape):
    """Both strides 0 on the batch file's layout (one path for all): the bytes of
    drcvar_mpc_step_advance_batch_f64 and of the mirror."""
    H, nx, nu = shape
    for n, (name, P, begin, rows, disturbed, steps) in enumerate(tb.plans(H)):
        cases = route_cases(H, nx, nu, P, begin, rows, disturbed, steps, 2 * n)
        problems = tb.make_problems(cases)
        pre, regions = tb.pack(problems)
        want, _ = tb.pack(tb.mirror(cases, problems))
        batch = tb.launch(cases, torch.from_numpy(pre).to(dev), regions)
        got = launch_route(cases, torch.from_numpy(pre).to(dev), regions, (0, 0))
        bad = tb.mismatches(cases, got, pre, want, regions)
        assert not bad, (cases[0], bad)
        assert got.tobytes() == batch.tobytes() == want.tobytes(), cases[0]
