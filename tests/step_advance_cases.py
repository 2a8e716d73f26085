"""The designed cases of tests/test_step_advance_gpu.py (drcvar_mpc_step_advance_f64 against
tests/step_advance_mirror.py), their inputs and the byte layout they are launched in.  Plain NumPy:
no engine, no device, so tests/test_step_advance_mirror.py can import the list and ask whether it
would notice a wrong kernel.

CASES maps a group name to a list of Case:

* ``windows-*``: one group per model shape; every path length of `path_lengths` crossed with every
  step of `steps`: the start, mid-path, the clamp at the path's end arriving row by row, the clamp
  at row 0 on both sides of the kernel's pre-clamp, and both ends of int64.  Logged at i = 1 of 3
  rows; disturbance, stream offset, status and have_last cycle along the list.
* ``logging``: i at 0, log_rows - 1, log_rows and -1, no log rows at all, and i = 1 by wrapping
  (step_begin = 2^63 - 1, step = -2^63), each with and without a disturbance, solved and unsolved.
* ``status``: every status of the header, a non-integer one and NaN, with and without a remembered
  optimum, at every shape.

Inputs are seeded normal draws with special values only where the launch copies them: -0.0 in
u_out, NaN in info[OBJECTIVE] and info[MAX_SLACK] on an unsolved step (and in info[STATUS] where
the case says so), inf in one entry of u_ref_path.  x_out[1] and the disturbance are finite, so the
one addition has a defined bit pattern.

Layout (`pack`): all buffers of a launch in one byte array, each starting on a 16-byte boundary
with at least GUARD_BYTES = 128 bytes (16 doubles; around have_last, 32 int32 words) of a sentinel
in its own type on both sides.  The logs are pre-filled with a second sentinel.
"""
import collections

import numpy as np

from step_advance_mirror import BUFFERS, INFO_WIDTH, INFO_STATUS, INPUTS, OUTPUTS, wrap_int64

INFO_OBJECTIVE, INFO_MAX_SLACK = 2, 6          # include/drcvar_mpc.h
SHAPES = [(1, 1, 1),      # no shifted row
          (10, 4, 2),     # the shape in use
          (30, 5, 4),     # H nu = 120
          (64, 8, 1),     # 520 window elements: three passes of the strided loop
          (64, 2, 4),     # all 256 threads own an input element
          (63, 8, 4)]     # 252 inputs, 512 window elements
OFFSETS = (3, 2 ** 32 - 1, 2 ** 64 - 1)
NAN = float("nan")
STATUSES = (0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 0.5, NAN)
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1

GUARD_BYTES = 128
GUARD_F64 = -1.2345678901234567e+77
GUARD_I32 = 0x5A5AA5A5
LOG_FILL = 9.87654321e-55

Case = collections.namedtuple(
    "Case", "H nx nu path_steps step step_begin log_rows disturbed offset status have_last seed")


def path_lengths(H):
    return (1, H, H + 1, 3 * H + 5)


def steps(H, P):
    s = [0, P // 2, *range(P - H - 2, P + 2), -1, -(H + 2), -(H + 3), INT64_MIN, INT64_MAX]
    return list(dict.fromkeys(s))


def _cases():
    groups, seed = {}, 0

    def add(group, **kw):
        nonlocal seed
        groups.setdefault(group, []).append(Case(seed=seed, **kw))
        seed += 1

    for H, nx, nu in SHAPES:
        n = 0
        for P in path_lengths(H):
            for s in steps(H, P):
                add(f"windows-H{H}-nx{nx}-nu{nu}", H=H, nx=nx, nu=nu, path_steps=P, step=s,
                    step_begin=wrap_int64(s - 1), log_rows=3, disturbed=bool(n % 2),
                    offset=OFFSETS[n % 3], status=(0.0, 1.0, 3.0, 4.0, 1.0)[n % 5],
                    have_last=(n // 2) % 2)
                n += 1
    for H, nx, nu in (SHAPES[0], SHAPES[1], SHAPES[3]):
        P, s = 3 * H + 5, H
        logging = [(s, wrap_int64(s - i), rows) for i, rows in ((0, 5), (4, 5), (5, 5), (-1, 5), (0, 0))]
        logging.append((INT64_MIN, INT64_MAX, 5))
        for step, begin, rows in logging:
            for disturbed in (False, True):
                for status in (0.0, 1.0):
                    add("logging", H=H, nx=nx, nu=nu, path_steps=P, step=step, step_begin=begin,
                        log_rows=rows, disturbed=disturbed, offset=OFFSETS[0], status=status,
                        have_last=1)
    for H, nx, nu in SHAPES:
        for status in STATUSES:
            for have_last in (0, 1):
                add("status", H=H, nx=nx, nu=nu, path_steps=3 * H + 5, step=2, step_begin=0,
                    log_rows=3, disturbed=True, offset=OFFSETS[0], status=status,
                    have_last=have_last)
    return groups


CASES = _cases()
N_LAUNCHES = sum(len(v) for v in CASES.values())


def log_index(case):
    """(i, logged) of the case, from the header's definition."""
    i = (case.step - case.step_begin) % 2 ** 64
    return i, i < case.log_rows


def solver_outputs(rng, H, nx, nu, status):
    """One scripted answer of the solver: (x_out, u_out, info)."""
    x_out = rng.standard_normal((H + 1, nx))
    u_out = rng.standard_normal((H, nu))
    u_out[0, 0] = -0.0
    if H > 1:
        u_out[1, nu - 1] = -0.0
    info = rng.standard_normal(INFO_WIDTH)
    info[INFO_STATUS] = status
    if not (status == 0.0 or status == 3.0):
        info[INFO_OBJECTIVE] = info[INFO_MAX_SLACK] = NAN
    return x_out, u_out, info


def make_buffers(case):
    """The pre-launch contents of every buffer (the mirror's ``buffers``) and the state."""
    c = case
    rng = np.random.default_rng(c.seed)
    b = {}
    b["x_out"], b["u_out"], b["info"] = solver_outputs(rng, c.H, c.nx, c.nu, c.status)
    b["x_ref_path"] = rng.standard_normal((c.path_steps, c.nx))
    b["u_ref_path"] = rng.standard_normal((c.path_steps, c.nu))
    b["u_ref_path"][rng.integers(c.path_steps), rng.integers(c.nu)] = np.inf
    b["disturbance"] = rng.standard_normal((c.log_rows, c.nx)) if c.disturbed else None
    b["x_log"] = np.full((c.log_rows + 1, c.nx), LOG_FILL)
    b["u_log"] = np.full((c.log_rows, c.nu), LOG_FILL)
    b["info_log"] = np.full((c.log_rows, INFO_WIDTH), LOG_FILL)
    b["x0"] = rng.standard_normal(c.nx)
    b["x_ref_win"] = rng.standard_normal((c.H + 1, c.nx))
    b["u_fallback"] = rng.standard_normal((c.H, c.nu))
    b["last_u"] = rng.standard_normal((c.H, c.nu))
    b["have_last"] = np.array([c.have_last], dtype=np.int32)
    return b, (c.offset, c.step)


# ---- the byte layout of one launch ---------------------------------------------------------------
def pack(buffers, state):
    """All buffers and the state in one uint8 array.  Returns ``(array, regions)`` with
    ``regions[name] = (byte offset, shape, dtype)``; a buffer that is None has no region."""
    items = [(n, np.ascontiguousarray(buffers[n])) for n in BUFFERS if buffers[n] is not None]
    items.append(("state", np.array([state[0], state[1] % 2 ** 64], dtype=np.uint64)))
    chunks, regions, at = [], {}, 0
    for name, a in items:
        guard = (np.full(GUARD_BYTES // 4, GUARD_I32, dtype=np.int32) if a.dtype == np.int32
                 else np.full(GUARD_BYTES // 8, GUARD_F64))
        pad = guard[:(-a.nbytes % 16) // guard.itemsize]
        regions[name] = (at + GUARD_BYTES, a.shape, a.dtype)
        for piece in (guard, a.reshape(-1), pad, guard):
            chunks.append(piece.view(np.uint8))
            at += piece.nbytes
        assert at % 16 == 0
    return np.concatenate(chunks), regions


def view(array, regions, name):
    at, shape, dtype = regions[name]
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    return array[at:at + n].view(dtype).reshape(shape)


def data_mask(array, regions):
    mask = np.zeros(array.shape, dtype=bool)
    for name in regions:
        at = regions[name][0]
        mask[at:at + view(array, regions, name).nbytes] = True
    return mask


def mismatches(case, got, pre, want, regions):
    """What a launch got wrong, as a list of strings (empty: nothing).  ``got``: the bytes after the
    launch; ``pre``: before it; ``want``: `pack` of the mirror's answer."""
    bad = []
    same = lambda a, b: a.tobytes() == b.tobytes()
    for name in OUTPUTS + ("state",):
        if not same(view(got, regions, name), view(want, regions, name)):
            bad.append(f"{name} differs from the mirror")
    guards = ~data_mask(pre, regions)
    if not same(got[guards], pre[guards]):
        at = np.flatnonzero(guards & (got != pre))
        bad.append(f"guard bytes written at {at[:8].tolist()} (regions {regions})")
    i, logged = log_index(case)
    for name, row in (("x_log", i + 1), ("u_log", i), ("info_log", i)):
        log, before = view(got, regions, name), view(pre, regions, name)
        others = [r for r in range(log.shape[0]) if not (logged and r == row)]
        # (what the row held before the launch: LOG_FILL, or an earlier launch's row in a chain)
        if not same(log[others], before[others]):
            bad.append(f"{name}: a row other than {row if logged else None} was written")
    for name in INPUTS:
        if name in regions and not same(view(got, regions, name), view(pre, regions, name)):
            bad.append(f"input {name} was modified")
    return bad


# ---- the scripted chain ----------------------------------------------------------------------------
CHAIN_SHAPES = [SHAPES[1], SHAPES[4]]
# unsolved, unsolved, solved, unsolved x3, inaccurate, unsolved, solved, solved, unsolved, unsolved
CHAIN_STATUSES = (1.0, 2.0, 0.0, 4.0, NAN, 0.5, 3.0, 5.0, 0.0, 0.0, 1.0, 2.0)


def chain(H, nx, nu):
    """``(case of the first launch, [solver outputs of launch r])``: 12 consecutive steps that
    start two steps before the path's end, every one logged and disturbed, with no optimum
    remembered at first, so that the reference inputs, a fresh shifted optimum and one shifted
    again while it goes stale are all rolled out."""
    P = 3 * H + 5
    first = Case(H=H, nx=nx, nu=nu, path_steps=P, step=P - 3, step_begin=P - 3,
                 log_rows=len(CHAIN_STATUSES), disturbed=True, offset=2 ** 64 - 5,
                 status=CHAIN_STATUSES[0], have_last=0, seed=10_000 + H * nu)
    rng = np.random.default_rng(first.seed + 1)
    return first, [solver_outputs(rng, H, nx, nu, st) for st in CHAIN_STATUSES]
