"""NumPy restatement of drcvar_loop_clearance_f64 (include/drcvar_loop_eval.h), per problem and with
the guards, built on tests/clearance_mirror.py: the noise a problem at path row s meets is
``clearance_mirror.noise(kind, params, O, T_n, M, seed, stream_offset)[:, :, s]``.  A helper of
tests/test_loop_clearance_gpu.py, never the product path.  np.minimum and ndarray.min propagate
NaN: min_d2 takes a NaN d^2 and keeps it, and the launch that met it counts nothing for it, which
is the entry's contract.
"""
import numpy as np

import clearance_mirror as cm

MASK64 = 2 ** 64 - 1


def evaluated(s, step_begin, log_rows, noise_steps):
    """The entry's guard: i = s - step_begin as the wrapped 64-bit difference, at most log_rows,
    and 0 <= s < noise_steps.  Returns i, or None when problem b is left alone."""
    i = (int(s) - int(step_begin)) & MASK64
    return i if i <= log_rows and 0 <= int(s) < noise_steps else None


def ego_of(c_out, x):
    """c_out x as a chain over j from +0.0 (exact for a selector, which the tests use)."""
    ego = np.zeros(2)
    for j in range(len(x)):
        ego = ego + np.asarray(c_out)[:, j] * x[j]
    return ego


def launch(x0, c_out, nominal_path, n_obstacles, steps, min_d2, step_hits, *, step_begin, log_rows,
           noise_steps, kind, params, combined_radius, seed, eval_offset, stride, zero_first_step):
    """One launch, in place on ``min_d2 [B, M]`` and ``step_hits [B, log_rows + 1]`` (or None).
    Returns (the smallest |min_o d^2 - R^2| over the evaluated problems, the list of log rows: i
    or None per problem)."""
    B, M = min_d2.shape
    O, P = n_obstacles, nominal_path.shape[1]
    rr = combined_radius * combined_radius
    margin, rows = np.inf, []
    for b in range(B):
        s = int(steps[b])
        i = evaluated(s, step_begin, log_rows, noise_steps)
        rows.append(i)
        if i is None:
            continue
        offset = (eval_offset + b * stride) & MASK64
        nz = cm.noise(kind, params, O, noise_steps, M, seed, offset, 0, zero_first_step)[:, :, s]
        row = min(max(s, 0), P - 1)
        pos = nominal_path[b * O:(b + 1) * O, row][None] + nz                   # [M, O, 2]
        d = ego_of(c_out, x0[b])[None, None] - pos
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).min(axis=1)        # [M]
        min_d2[b] = np.minimum(min_d2[b], d2)
        if step_hits is not None:
            step_hits[b, i] += int((d2 < rr).sum())
        margin = min(margin, float(np.min(np.abs(d2 - rr))))
    return margin, rows
