"""GPU: drcvar_mpc_step_advance_batch_f64 (csrc/drcvar_step.hip) against
tests/step_advance_mirror.py applied to each problem's slices, BIT FOR BIT: the launch is copies
plus one IEEE addition of finite numbers per state element, so there is no tolerance in this file.

A launch of B problems goes through the C entry with a bare drcvar_mpc_model on one device
allocation that holds every buffer, stacked over the problems, between the sentinel guards of
tests/step_advance_cases.py, the B states as one [B, 2] array on a 16-byte boundary.  The mirror
runs once per problem with that problem's state, info, have_last and disturbance (the paths are
shared); `pack` of its stacked answers is what the allocation must hold afterwards.  Compared as
bytes (`mismatches`): every output buffer and all B states; every guard byte; every log row of
every problem other than the one that problem wrote; every input buffer (unchanged) — and, last,
the whole allocation at once.

Shapes: (1, 1, 1), (10, 4, 2) and the ABI's limits (64, 8, 4) — 256 threads own an input element,
520 window elements take three passes — at B = 1, 2, 5 and 300 (more workgroups than the device
has compute units).  Inside ONE launch the problems differ in everything that is per problem, which
is what a kernel that reads problem 0's words for everyone gets wrong: statuses (every one of the
header, a non-integer, NaN), have_last, the step (the start, the last log row, one past the log
rows, one before them, the path's last row, one past the path's end, further past it, negative on
both sides of the kernel's pre-clamp) and the stream offset (the carries at 2^32 and 2^64).  The
`plans` cross that with a disturbance present and NULL, no log rows at all, and paths shorter than
the window (P = H and P = 1).  At B = 2 the two steps are +-2^63.

The scripted chain is 12 consecutive launches of B = 3 on one allocation: problem b follows
test_step_advance_gpu.py's solved/unsolved script shifted by b (and its own stream offset), the
solver's outputs of launch r are copied in before it, and the allocation is compared with the
iterated mirror after every launch.
"""
import ctypes

import numpy as np
import pytest
import torch

import step_advance_cases as sc
import step_advance_mirror as sm
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native

pytestmark = pytest.mark.gpu
ARGUMENTS = ("x_out", "u_out", "info", "x_ref_path", "u_ref_path")
FIXED = ("x_log", "u_log", "info_log", "x0", "x_ref_win", "u_fallback", "last_u", "have_last", "state")
SHARED = ("x_ref_path", "u_ref_path")
SHAPES = [(1, 1, 1), (10, 4, 2), (64, 8, 4)]
BATCHES = (1, 2, 5, 300)
OFFSETS = (3, 2 ** 32 - 1, 2 ** 64 - 1, 2 ** 32, 12345)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


# ---- a launch of B problems: per-problem cases over shared paths -----------------------------------
def plans(H):
    """(name, path_steps, step_begin, log_rows, disturbed, the steps the problems cycle through)."""
    P, begin = 3 * H + 5, 7
    varied = [begin, begin + 1, begin + 3, begin + 4, begin - 1, P - 1, P, P + 3, -1, -(H + 2), -(H + 3)]
    return [("disturbed", P, begin, 4, True, varied),
            ("undisturbed-short-path", H, begin, 4, False, varied),
            ("no-log-rows-one-row-path", 1, begin, 0, False, varied)]


def batch_cases(H, nx, nu, B, P, begin, rows, disturbed, steps, shift=0):
    """Problem b's Case: step, offset, status and have_last cycle with periods 11, 5, 8 and 3."""
    return [sc.Case(H=H, nx=nx, nu=nu, path_steps=P, step=steps[(b + shift) % len(steps)],
                    step_begin=begin, log_rows=rows, disturbed=disturbed,
                    offset=OFFSETS[(b + shift) % len(OFFSETS)],
                    status=sc.STATUSES[(b + shift) % len(sc.STATUSES)],
                    have_last=int((b + shift) % 3 == 1), seed=50_000 + 1000 * shift + b)
            for b in range(B)]


def make_problems(cases):
    """[(buffers, state)] per problem, the paths of problem 0 shared by all."""
    problems = [sc.make_buffers(c) for c in cases]
    for buffers, _ in problems[1:]:
        for name in SHARED:
            buffers[name] = problems[0][0][name]
    return problems


def pack(problems):
    """`step_advance_cases.pack` of a batch: every per-problem buffer stacked to [B, ...], the
    shared paths once, the states as uint64 [B, 2].  Returns ``(bytes, regions)``."""
    first = problems[0][0]
    items = []
    for name in sm.BUFFERS:
        if first[name] is None:
            continue
        if name in SHARED:
            items.append((name, np.ascontiguousarray(first[name])))
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


def mirror(cases, problems):
    return [sm.step_advance(buffers, c.H, c.nx, c.nu, c.path_steps, c.step_begin, c.log_rows, state)
            for c, (buffers, state) in zip(cases, problems)]


def launch(cases, arena, regions):
    """One launch on the device bytes `arena`; a buffer without a region (no disturbance) is NULL."""
    c = cases[0]
    assert arena.data_ptr() % 16 == 0 and regions["state"][0] % 16 == 0
    model = _native.MpcModel()
    model.horizon, model.n_states, model.n_inputs, model.n_outputs = c.H, c.nx, c.nu, 2
    at = lambda name: ctypes.c_void_p(arena.data_ptr() + regions[name][0] if name in regions else None)
    stream = torch.cuda.current_stream(arena.device).cuda_stream
    rc = _native.loop_lib().drcvar_mpc_step_advance_batch_f64(
        ctypes.byref(model), len(cases), *(at(n) for n in ARGUMENTS), c.path_steps, at("disturbance"),
        c.step_begin, c.log_rows, *(at(n) for n in FIXED), ctypes.c_void_p(stream))
    assert rc == _native.OK, c
    return arena.cpu().numpy()


def mismatches(cases, got, pre, want, regions):
    """What a launch got wrong, as a list of strings (empty: nothing)."""
    bad = []
    same = lambda a, b: a.tobytes() == b.tobytes()
    for name in sm.OUTPUTS + ("state",):
        g, w = sc.view(got, regions, name), sc.view(want, regions, name)
        wrong = [b for b in range(len(cases)) if not same(g[b], w[b])]
        if wrong:
            bad.append(f"{name} differs from the mirror in problems {wrong[:8]}")
    guards = ~sc.data_mask(pre, regions)
    if not same(got[guards], pre[guards]):
        bad.append(f"guard bytes written at {np.flatnonzero(guards & (got != pre))[:8].tolist()}")
    for name, shift in (("x_log", 1), ("u_log", 0), ("info_log", 0)):
        log, before = sc.view(got, regions, name), sc.view(pre, regions, name)
        for b, c in enumerate(cases):
            i, logged = sc.log_index(c)
            others = [r for r in range(log.shape[1]) if not (logged and r == i + shift)]
            if not same(log[b][others], before[b][others]):
                bad.append(f"{name}[{b}]: a row other than {i + shift if logged else None} was written")
    for name in sm.INPUTS:
        if name in regions and not same(sc.view(got, regions, name), sc.view(pre, regions, name)):
            bad.append(f"input {name} was modified")
    if not bad and not same(got, want):
        bad.append("the allocations differ")
    return bad


def check_launch(dev, cases):
    problems = make_problems(cases)
    pre, regions = pack(problems)
    want, _ = pack(mirror(cases, problems))
    got = launch(cases, torch.from_numpy(pre).to(dev), regions)
    bad = mismatches(cases, got, pre, want, regions)
    assert not bad, (cases[0], len(cases), bad)


def test_the_plans_hold_what_they_claim():
    """(needs no device) at B = 300 one launch holds every status, both have_last values, every
    offset with its carry, and steps that are logged, outside the log rows on both sides, past the
    path's end and negative."""
    H = 10
    name, P, begin, rows, disturbed, steps = plans(H)[0]
    cases = batch_cases(H, 4, 2, 300, P, begin, rows, disturbed, steps)
    assert {repr(c.status) for c in cases} == {repr(s) for s in sc.STATUSES}
    assert {c.have_last for c in cases} == {0, 1} and {c.offset for c in cases} == set(OFFSETS)
    assert {2 ** 32 - 1, 2 ** 64 - 1} <= set(OFFSETS)
    index = [sc.log_index(c) for c in cases]
    assert {i for i, logged in index if logged} == {0, 1, 3}
    assert any(i == rows for i, _ in index) and any(i == 2 ** 64 - 1 for i, _ in index)
    assert {P, P + 3, -1, -(H + 3)} <= {c.step for c in cases}
    assert [p[1] for p in plans(H)] == [3 * H + 5, H, 1] and plans(H)[2][3] == 0
    assert [p[4] for p in plans(H)] == [True, False, False]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H%d-nx%d-nu%d" % s)
def test_batch_equals_the_mirror_per_problem(dev, shape, B):
    H, nx, nu = shape
    for n, (name, P, begin, rows, disturbed, steps) in enumerate(plans(H)):
        for shift in ((0, 4) if B < 5 else (0,)):      # few problems: a second slice of the cycles
            check_launch(dev, batch_cases(H, nx, nu, B, P, begin, rows, disturbed, steps, shift + n))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "H%d-nx%d-nu%d" % s)
def test_the_ends_of_int64_side_by_side(dev, shape):
    """B = 2 with steps -2^63 and 2^63 - 1 and step_begin = 2^63 - 1: problem 0 logs row 1 by
    wrapping, problem 1 row 0; every window row is the path's first / last one; the stored steps
    wrap to -2^63 + 1 and -2^63."""
    H, nx, nu = shape
    for disturbed in (False, True):
        cases = batch_cases(H, nx, nu, 2, 3 * H + 5, sc.INT64_MAX, 3, disturbed,
                            [sc.INT64_MIN, sc.INT64_MAX])
        assert [sc.log_index(c) for c in cases] == [(1, True), (0, True)]
        check_launch(dev, cases)
        check_launch(dev, cases[::-1])


@pytest.mark.parametrize("shape", sc.CHAIN_SHAPES, ids=lambda s: "H%d-nx%d-nu%d" % s)
def test_scripted_chain_of_three_problems(dev, shape):
    H, nx, nu = shape
    B, n = 3, len(sc.CHAIN_STATUSES)
    P = 3 * H + 5
    script = [[sc.CHAIN_STATUSES[(r + b) % n] for r in range(n)] for b in range(B)]
    offsets = (2 ** 64 - 5, 2 ** 32 - 5, 7)
    cases = [sc.Case(H=H, nx=nx, nu=nu, path_steps=P, step=P - 3, step_begin=P - 3, log_rows=n,
                     disturbed=True, offset=offsets[b], status=script[b][0], have_last=0,
                     seed=20_000 + 10 * H * nu + b) for b in range(B)]
    rngs = [np.random.default_rng(c.seed + 1) for c in cases]
    problems = make_problems(cases)
    pre, regions = pack(problems)
    arena = torch.from_numpy(pre).to(dev)
    for r in range(n):
        answers = [sc.solver_outputs(rngs[b], H, nx, nu, script[b][r]) for b in range(B)]
        problems = [(dict(buffers, x_out=x, u_out=u, info=info), state)
                    for (buffers, state), (x, u, info) in zip(problems, answers)]
        pre, _ = pack(problems)
        for name in ("x_out", "u_out", "info"):
            lo = regions[name][0]
            hi = lo + sc.view(pre, regions, name).nbytes
            arena[lo:hi].copy_(torch.from_numpy(pre[lo:hi]))
        cases = [c._replace(step=state[1], status=float(script[b][r]))
                 for b, (c, (_, state)) in enumerate(zip(cases, problems))]
        after = mirror(cases, problems)
        want, _ = pack(after)
        got = launch(cases, arena, regions)
        bad = mismatches(cases, got, pre, want, regions)
        assert not bad, (r, bad)
        assert got.tobytes() == want.tobytes(), r
        problems = after
    for b, (buffers, state) in enumerate(problems):
        assert state == ((offsets[b] + n) % 2 ** 64, P - 3 + n)
        assert int(buffers["have_last"][0]) == 1
