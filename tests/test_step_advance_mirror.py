"""CPU: tests/step_advance_mirror.py (the contract of drcvar_mpc_step_advance_f64 in plain Python)
against the oracle's fallback inputs and two hand-worked steps, and the case list of
tests/test_step_advance_gpu.py against sixteen wrong mirrors.

The last is a condition, not a measurement: `_variant` restates the mirror with one deliberate
error per number (``wrong=None`` is the mirror itself, which a test pins on every case), and for
each error at least one GPU case must give different bytes in some output buffer, and the
comparison the GPU test makes (`step_advance_cases.mismatches`) must report it.
"""
import functools

import numpy as np
import pytest

import step_advance_cases as sc
import step_advance_mirror as sm
from oracle import mpc_qp

NAN = float("nan")


def _run(case, mirror=sm.step_advance):
    buffers, state = sc.make_buffers(case)
    return mirror(buffers, case.H, case.nx, case.nu, case.path_steps, case.step_begin,
                  case.log_rows, state)


# ---- the fallback inputs against the oracle ----------------------------------------------------
@pytest.mark.parametrize("H,nu", [(1, 1), (1, 3), (2, 1), (4, 2), (10, 2)])
@pytest.mark.parametrize("status", [0.0, 3.0, 1.0])
@pytest.mark.parametrize("have_last", [0, 1])
def test_fallback_equals_the_oracle(H, nu, status, have_last):
    P = 3 * H + 5
    for step in (0, 3, P - H - 1):          # s' + H - 1 <= P - 1: the window is inside the path
        case = sc.Case(H=H, nx=2, nu=nu, path_steps=P, step=step, step_begin=0, log_rows=0,
                       disturbed=False, offset=0, status=status, have_last=have_last, seed=H + nu)
        buffers, _ = sc.make_buffers(case)
        out, _ = _run(case)
        solved = status in (0.0, 3.0)
        last = buffers["u_out"] if solved else (buffers["last_u"] if have_last else None)
        window = buffers["u_ref_path"][step + 1:step + 1 + H]
        want = mpc_qp.fallback_inputs(H, nu, window, last)
        assert out["u_fallback"].tobytes() == np.asarray(want, dtype=np.float64).tobytes()
        assert out["have_last"][0] == int(solved or have_last)
        assert out["last_u"].tobytes() == (buffers["u_out"] if solved else buffers["last_u"]).tobytes()


# ---- hand-worked steps: H = 2, nx = 1, nu = 1, path_steps = 3 ----------------------------------
def _hand(status, have_last, last_u):
    col = lambda *v: np.array(v, dtype=np.float64).reshape(-1, 1)
    info = np.arange(10, dtype=np.float64)
    info[0] = status
    return dict(x_out=col(10, 11, 12), u_out=col(0.5, 0.25), info=info,
                x_ref_path=col(100, 101, 102), u_ref_path=col(1, 2, 3),
                disturbance=col(0.125, 0.0625), x_log=col(-1, -1, -1), u_log=col(-1, -1),
                info_log=np.full((2, 10), -1.0), x0=np.array([-2.0]), x_ref_win=col(-3, -3, -3),
                u_fallback=col(-4, -4), last_u=col(*last_u),
                have_last=np.array([have_last], dtype=np.int32)), info


def _equal(out, **want):
    for name, w in want.items():
        got = out[name]
        assert got.dtype == (np.int32 if name == "have_last" else np.float64), name
        assert got.reshape(-1).tolist() == w, name


def test_hand_worked_solved_step():
    """s = 1, i = 1: logged into the last row; s' = 2 and the whole window is the last path row;
    the solved answer is remembered and shifted, its tail filled from c(s' + 1) = 2."""
    b, info = _hand(status=0.0, have_last=0, last_u=(9, 8))
    out, state = sm.step_advance(b, 2, 1, 1, 3, 0, 2, (7, 1))
    _equal(out, x_log=[-1, -1, 11.0625], u_log=[-1, 0.5],
           info_log=[-1.0] * 10 + info.tolist(), last_u=[0.5, 0.25], have_last=[1],
           x0=[11.0625], x_ref_win=[102, 102, 102], u_fallback=[0.25, 3.0],
           x_out=[10, 11, 12], u_out=[0.5, 0.25], info=info.tolist(),
           x_ref_path=[100, 101, 102], u_ref_path=[1, 2, 3], disturbance=[0.125, 0.0625])
    assert state == (8, 2)


def test_hand_worked_unsolved_step():
    """s = -1 = step_begin, i = 0; s' = 0; nothing remembered: the reference inputs; the offset
    wraps at 2^64."""
    b, info = _hand(status=1.0, have_last=0, last_u=(9, 8))
    out, state = sm.step_advance(b, 2, 1, 1, 3, -1, 2, (2 ** 64 - 1, -1))
    _equal(out, x_log=[-1, 11.125, -1], u_log=[0.5, -1],
           info_log=info.tolist() + [-1.0] * 10, last_u=[9, 8], have_last=[0],
           x0=[11.125], x_ref_win=[100, 101, 102], u_fallback=[1.0, 2.0])
    assert state == (0, 0)
    # the same step with a stale optimum: shifted, the tail from c(s' + 1) = 1
    b, _ = _hand(status=1.0, have_last=1, last_u=(9, 8))
    out, _ = sm.step_advance(b, 2, 1, 1, 3, -1, 2, (2 ** 64 - 1, -1))
    _equal(out, last_u=[9, 8], have_last=[1], u_fallback=[8.0, 2.0])
    # not logged (i = 2 = log_rows): no log row, no disturbance, the state still advances
    b, _ = _hand(status=1.0, have_last=0, last_u=(9, 8))
    out, state = sm.step_advance(b, 2, 1, 1, 3, -3, 2, (5, -1))
    _equal(out, x_log=[-1, -1, -1], u_log=[-1, -1], info_log=[-1.0] * 20, x0=[11.0])
    assert state == (6, 0)


def test_step_wraps_and_windows_do_not():
    b, _ = _hand(status=1.0, have_last=0, last_u=(9, 8))
    out, state = sm.step_advance(b, 2, 1, 1, 3, 0, 0, (0, 2 ** 63 - 1))
    assert state == (1, -2 ** 63)
    _equal(out, x_ref_win=[102, 102, 102], u_fallback=[3.0, 3.0])
    out, state = sm.step_advance(b, 2, 1, 1, 3, 0, 0, (0, -2 ** 63))
    assert state == (1, -2 ** 63 + 1)
    _equal(out, x_ref_win=[100, 100, 100], u_fallback=[1.0, 1.0])


# ---- the wrong mirrors ---------------------------------------------------------------------------
WRONG = {
    1: "the disturbance is added when the step is not logged",
    2: "on a solved step the shift reads the old last_u instead of u_out",
    3: "the last fallback row is taken from c(s' + H)",
    4: "the windows are taken from c(s + k)",
    5: "status 3 is counted as unsolved",
    6: "status 1 is counted as solved",
    7: "have_last is set on every step",
    8: "last_u is overwritten on an unsolved step",
    9: "x_log row i is written instead of i + 1",
    10: "i ignores step_begin",
    11: "stream_offset is incremented in its low 32 bits only",
    12: "only the first 256 elements of x_ref_win are written",
    13: "only the first 120 elements of u_fallback / last_u are written",
    14: "the state is not advanced on an unlogged step",
    15: "step saturates instead of wrapping at 2^63 - 1",
    16: "the low clamp is missing: rows below 0 are taken as row path_steps - 1",
}


def _variant(wrong, b, H, nx, nu, path_steps, step_begin, log_rows, state):
    out = {name: None if b[name] is None else np.array(b[name], copy=True) for name in sm.BUFFERS}
    offset, s = state

    def c(r):
        if wrong == 16 and r < 0:
            return path_steps - 1
        return min(max(r, 0), path_steps - 1)

    first = s if wrong == 4 else s + 1
    i = (s if wrong == 10 else s - step_begin) % 2 ** 64
    logged = i < log_rows
    x_next = np.array(b["x_out"][1], copy=True)
    if b["disturbance"] is not None:
        if logged:
            x_next = x_next + b["disturbance"][i]
        elif wrong == 1 and log_rows > 0:
            x_next = x_next + b["disturbance"][i % log_rows]
    if logged:
        out["x_log"][i if wrong == 9 else i + 1] = x_next
        out["u_log"][i] = b["u_out"][0]
        out["info_log"][i] = b["info"]
    status = float(b["info"][sm.INFO_STATUS])
    solved = status == 0.0 or (status == 3.0 and wrong != 5) or (status == 1.0 and wrong == 6)
    if solved or wrong == 8:
        out["last_u"][...] = b["u_out"]
    if solved or wrong == 7:
        out["have_last"][0] = 1
    have = solved or int(b["have_last"][0]) != 0
    out["x0"][...] = x_next
    for k in range(H + 1):
        out["x_ref_win"][k] = b["x_ref_path"][c(first + k)]
    shift_from = b["last_u"] if wrong == 2 else out["last_u"]
    for k in range(H):
        if have and k < H - 1:
            out["u_fallback"][k] = shift_from[k + 1]
        elif have and wrong == 3:
            out["u_fallback"][k] = b["u_ref_path"][c(first + H)]
        else:
            out["u_fallback"][k] = b["u_ref_path"][c(first + k)]
    if wrong == 12:
        out["x_ref_win"].reshape(-1)[256:] = b["x_ref_win"].reshape(-1)[256:]
    if wrong == 13:
        for name in ("u_fallback", "last_u"):
            out[name].reshape(-1)[120:] = b[name].reshape(-1)[120:]
    if wrong == 14 and not logged:
        return out, (offset, s)
    if wrong == 11:
        offset = (offset & ~0xFFFFFFFF) | ((offset + 1) & 0xFFFFFFFF)
    else:
        offset = (offset + 1) % 2 ** 64
    step = min(s + 1, 2 ** 63 - 1) if wrong == 15 else sm.wrap_int64(s + 1)
    return out, (offset, step)


def _all_cases():
    return [c for group in sc.CASES.values() for c in group]


def _packed(case, wrong=None):
    mirror = sm.step_advance if wrong is None else (lambda *a: _variant(wrong, *a))
    return sc.pack(*_run(case, mirror))


@functools.lru_cache(maxsize=None)
def _right(seed):
    """(bytes before the launch, the mirror's bytes after it) of the case with this seed."""
    case = next(c for c in _all_cases() if c.seed == seed)
    return sc.pack(*sc.make_buffers(case))[0], _packed(case)[0]


def test_case_list_is_the_designed_one():
    assert sc.N_LAUNCHES <= 1500
    cases = _all_cases()
    assert {(c.H, c.nx, c.nu) for c in cases} == set(sc.SHAPES)
    assert {c.offset for c in cases} == {3, 2 ** 32 - 1, 2 ** 64 - 1}
    for H, nx, nu in sc.SHAPES:
        mine = [c for c in sc.CASES[f"windows-H{H}-nx{nx}-nu{nu}"]]
        assert {c.path_steps for c in mine} == {1, H, H + 1, 3 * H + 5}
        for P in (1, H, H + 1, 3 * H + 5):
            at = {c.step for c in mine if c.path_steps == P}
            assert at >= {0, P // 2, -1, -(H + 2), -(H + 3), -2 ** 63, 2 ** 63 - 1}
            assert at >= set(range(P - H - 2, P + 2))
        seen = {(repr(c.status), c.have_last) for c in sc.CASES["status"] if (c.H, c.nx, c.nu) == (H, nx, nu)}
        assert seen == {(repr(st), h) for st in (0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 0.5, NAN) for h in (0, 1)}
    logging = {(sc.log_index(c)[0], c.log_rows, c.disturbed) for c in sc.CASES["logging"]}
    for d in (False, True):
        assert logging >= {(0, 5, d), (4, 5, d), (5, 5, d), (2 ** 64 - 1, 5, d), (0, 0, d), (1, 5, d)}
    assert any(c.step == -2 ** 63 and c.step_begin == 2 ** 63 - 1 for c in sc.CASES["logging"])


def test_variant_without_an_error_is_the_mirror():
    for case in _all_cases():
        got, _ = _packed(case, wrong=0)
        want = _right(case.seed)[1]
        assert got.tobytes() == want.tobytes(), case


def test_the_comparison_accepts_the_mirror_and_sees_every_region():
    """`mismatches` is empty for the mirror's own bytes and reports a flipped byte anywhere: in
    any buffer, the state, or a guard."""
    case = sc.CASES["logging"][3]           # logged, disturbed
    pre, regions = sc.pack(*sc.make_buffers(case))
    want, _ = _packed(case)
    assert sc.mismatches(case, want, pre, want, regions) == []
    for at in range(0, want.size, 8):
        got = want.copy()
        got[at] ^= 1
        assert sc.mismatches(case, got, pre, want, regions), at
    for name, (at, shape, dtype) in regions.items():
        assert at % 16 == 0, name
        guard = sc.GUARD_I32 if dtype == np.int32 else sc.GUARD_F64
        n = sc.view(pre, regions, name).nbytes
        before = pre[at - sc.GUARD_BYTES:at].view(dtype if dtype == np.int32 else np.float64)
        after = pre[at + n + (-n % 16):at + n + (-n % 16) + sc.GUARD_BYTES].view(before.dtype)
        assert before.size >= 16 and (before == guard).all() and (after == guard).all(), name


@pytest.mark.parametrize("wrong", list(WRONG), ids=lambda w: f"{w}-{WRONG[w].replace(' ', '_')[:40]}")
def test_case_list_catches_the_wrong_mirror(wrong):
    for case in _all_cases():
        got, regions = _packed(case, wrong)
        pre, want = _right(case.seed)
        if got.tobytes() != want.tobytes():
            assert sc.mismatches(case, got, pre, want, regions), (WRONG[wrong], case)
            return
    pytest.fail(f"no GPU case notices a kernel in which {WRONG[wrong]}")


def test_chain_script():
    assert len(sc.CHAIN_STATUSES) == 12
    solved = [st in (0.0, 3.0) for st in sc.CHAIN_STATUSES]
    assert solved == [False, False, True, False, False, False, True, False, True, True, False, False]
    assert sc.CHAIN_STATUSES[6] == 3.0
    for shape in sc.CHAIN_SHAPES:
        first, table = sc.chain(*shape)
        assert first.step == first.path_steps - 3 and len(table) == 12 and first.have_last == 0
