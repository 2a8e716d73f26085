"""drcvar_mpc_step_advance_f64 in plain Python, written from the header's steps 1-7
(include/drcvar_mpc.h), not from the kernel: the reference of tests/test_step_advance_gpu.py.

The launch is copies plus one IEEE addition, so with exact Python integers for every index and
NumPy float64 for the one sum this mirror is a bit-for-bit reference: compare as bytes.

``buffers`` maps the header's names to NumPy arrays holding the pre-launch contents:

    x_out [H+1, nx], u_out [H, nu], info [10], x_ref_path [P, nx], u_ref_path [P, nu],
    disturbance [log_rows, nx] or None                                         (read-only)
    x_log [log_rows+1, nx], u_log [log_rows, nu], info_log [log_rows, 10],
    x0 [nx], x_ref_win [H+1, nx], u_fallback [H, nu], last_u [H, nu]           (float64)
    have_last [1]                                                              (int32)

``state`` is ``(stream_offset, step)`` as Python ints, the offset in [0, 2^64), the step in
[-2^63, 2^63).  Returns ``(buffers after the launch, state after the launch)``; the input arrays
are not modified.
"""
import numpy as np

INFO_WIDTH, INFO_STATUS = 10, 0
INPUTS = ("x_out", "u_out", "info", "x_ref_path", "u_ref_path", "disturbance")
OUTPUTS = ("x_log", "u_log", "info_log", "x0", "x_ref_win", "u_fallback", "last_u", "have_last")
BUFFERS = INPUTS + OUTPUTS


def wrap_int64(v):
    """The int64 with the bit pattern of ``v mod 2^64``."""
    v %= 2 ** 64
    return v - 2 ** 64 if v >= 2 ** 63 else v


def step_advance(buffers, H, nx, nu, path_steps, step_begin, log_rows, state):
    b = buffers
    out = {name: None if b[name] is None else np.array(b[name], copy=True) for name in BUFFERS}
    offset, s = state

    def c(r):                               # row of a path; r is an unbounded integer
        return min(max(r, 0), path_steps - 1)

    i = (s - step_begin) % 2 ** 64          # the wrapped difference
    logged = i < log_rows
    # 1. next state
    x_next = np.array(b["x_out"][1], copy=True)
    if logged and b["disturbance"] is not None:
        x_next = x_next + b["disturbance"][i]
    # 2. log
    if logged:
        out["x_log"][i + 1] = x_next
        out["u_log"][i] = b["u_out"][0]
        out["info_log"][i] = b["info"]
    # 3. fallback memory
    status = float(b["info"][INFO_STATUS])
    solved = status == 0.0 or status == 3.0
    if solved:
        out["last_u"][...] = b["u_out"]
        out["have_last"][0] = 1
    have = solved or int(b["have_last"][0]) != 0
    # 4. next x0
    out["x0"][...] = x_next
    # 5. next reference window: rows c(s' + k) of the unwrapped s' = s + 1
    for k in range(H + 1):
        out["x_ref_win"][k] = b["x_ref_path"][c(s + 1 + k)]
    # 6. next fallback inputs
    for k in range(H):
        if have and k < H - 1:
            out["u_fallback"][k] = out["last_u"][k + 1]
        else:
            out["u_fallback"][k] = b["u_ref_path"][c(s + 1 + k)]
    # 7. state
    return out, ((offset + 1) % 2 ** 64, wrap_int64(s + 1))
