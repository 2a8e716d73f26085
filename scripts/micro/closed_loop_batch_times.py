"""Times a batch of receding-horizon loops (simulation/closed_loop.py, RecedingHorizonBatch) against
the single loop, and writes profiles/closed_loop/closed_loop_batch_times.json.

    python scripts/micro/closed_loop_batch_times.py --part single [--tree DIR] --out FILE
    python scripts/micro/closed_loop_batch_times.py [--out FILE] --ab-parent FILE ... --ab-tree FILE ...

Every figure is device-event time over a window of `--steps` back-to-back control steps after a
warm-up window: the median and the spread (min, max) of `--repeats` windows, in ms per control
step; loop-steps/s = B / time per control step.  Shape: main.py's (3 obstacles, H = 30, N = 20,
P = 151), problem b started from the scenario's start plus a small offset of its own.

  --part single   only RecedingHorizonFilter on `graph` with 10 steps per graph, importing the
                  package from --tree: run on a build of the parent commit and on this tree,
                  alternated in one session (parent, tree, parent, tree), and hand the files to
                  the full run with --ab-parent / --ab-tree
  (full run)      the single loop again, then RecedingHorizonBatch at B = 1, 8, 64, 256, 1024 on
                  `graph` (1 and 10 steps per graph) and on `launches`, then at B = 1024 each of a
                  step's three launches alone, replayed from a graph of one launch

The full run also states the two directions the batch was built for: the batch's loop-steps/s at
B = 64, 256 and 1024 exceed the single loop's with no overlap of the windows' ranges, and this
tree's single loop is within the spread of the parent's.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--part", choices=("all", "single"), default="all")
ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
ap.add_argument("--ab-parent", nargs="*", default=[])
ap.add_argument("--ab-tree", nargs="*", default=[])
ap.add_argument("--launches", type=int, default=10)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
REPO = os.path.abspath(args.tree)
sys.path.insert(0, REPO)

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.config.scenarios import (  # noqa: E402
    get_scenario_config)
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core.mpc_filter import (  # noqa: E402
    MPCModel, filter_batch)
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import closed_loop  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import obstacles as ob  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.planner import (  # noqa: E402
    ReferenceTrajectoryPlanner)

SEED, H, N, P, DT = 5, 30, 20, 151, 0.2
BATCHES = (1, 8, 64, 256, 1024)
REQUIRED = (64, 256, 1024)


def spread(ms, problems=1):
    ms = np.asarray(ms)
    rate = problems / (ms * 1e-3)
    return {"ms": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max()),
            "loop_steps_per_s": float(np.median(rate)), "loop_steps_per_s_min": float(rate.min()),
            "loop_steps_per_s_max": float(rate.max())}


def setup(dev):
    m = np.load(os.path.join(REPO, "tests", "golden", "mpc_multi_obstacle_h30.npz"), allow_pickle=False)
    cfg = get_scenario_config("multi_obstacle")
    planner = ReferenceTrajectoryPlanner(m["A"], m["B"], m["C"], m["Q"], m["R"], P, DT)
    x_ref, u_ref, _ = planner.straight_line_trajectory(cfg["ego_start"], cfg["ego_goal"])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    nominal = to(np.stack([ob.generate_nominal_trajectory(o["start"], o["direction"], o["speed"], P, DT)[:P]
                           for o in cfg["obstacles"]]))
    model = MPCModel(m["A"], m["B"], m["C"], m["Q"], m["R"], H, tuple(m["u_bounds"]),
                     tuple(m["p_bounds"]), device=dev)
    x0 = np.zeros(4)
    x0[:2] = cfg["ego_start"]
    return model, nominal, to(x_ref[:P]), to(u_ref[:P]), x0


def starts(x0, B):
    offsets = 1e-2 * np.random.default_rng(11).standard_normal((B, 4))
    offsets[0] = 0.0
    return x0 + offsets


def loop_windows(loop, x0, backend, problems=1):
    """ms per control step of `--repeats` windows of `--steps` steps, each from a reset."""
    result = []
    loop.reset(x0)
    result[:] = loop.run(args.steps, backend=backend)        # captures / warms up
    ms = []
    for _ in range(args.repeats):
        loop.reset(x0)                                       # same first step: the capture is kept
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        result[:] = loop.run(args.steps, backend=backend)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / args.steps)
    row = spread(ms, problems)
    status = result[2][..., 0]
    row["solved_share"] = float(((status == 0) | (status == 3)).double().mean())
    row["mean_iterations"] = float(result[2][..., 1].mean())
    return row


def single_row(dev, parts):
    model, nominal, x_ref, u_ref, x0 = parts
    loop = closed_loop.RecedingHorizonFilter(model, nominal, x_ref, u_ref, N, RiskParams(), seed=SEED,
                                             steps_per_graph=10)
    return loop_windows(loop, x0, "graph")


def graph_of(launch, side, dev):
    """A graph of the one launch `launch` issues on `side` (run once eagerly first)."""
    with torch.cuda.stream(side):
        launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch()
    return graph.replay


def timed(fn, before, problems):
    """ms per call of fn: windows of `--launches` back-to-back calls between two device events."""
    for _ in range(3):
        fn()
    ms = []
    for _ in range(args.repeats):
        before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / args.launches)
    return spread(ms, problems)


def launches_alone(dev, parts, B):
    """Each of a step's three launches alone at B problems, from the first step's buffers (every
    window starts from a reset, so the advance launch logs each of its steps)."""
    model, nominal, x_ref, u_ref, x0 = parts
    loop = closed_loop.RecedingHorizonBatch(model, nominal, x_ref, u_ref, N, RiskParams(),
                                            n_problems=B, seed=SEED)
    x0 = starts(x0, B)
    loop.reset(x0)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    halfspaces, _ = engine.prepare_sampled_halfspaces_dev(
        loop.nominal_path, loop.ego_path, H, N, RiskParams(), loop._state[0], seed=SEED,
        out=loop._record, stream=side)
    hs_h, hs_g = loop._views(loop._record)
    solver = lambda: filter_batch(model, hs_h, hs_g, loop._x0, loop._x_ref_win, loop._u_fb,
                                  workspace=loop._workspace, stream=side,
                                  out=(loop._x, loop._u, loop._info))
    vp = ctypes.c_void_p
    x_log, u_log, info_log = loop._logs
    advance = engine.PreparedLaunch(_native.loop_lib().drcvar_mpc_step_advance_batch_f64, (
        ctypes.pointer(model.model), B, vp(loop._x.data_ptr()), vp(loop._u.data_ptr()),
        vp(loop._info.data_ptr()), vp(x_ref.data_ptr()), vp(u_ref.data_ptr()), P, vp(None), 0,
        loop._cap, vp(x_log.data_ptr()), vp(u_log.data_ptr()), vp(info_log.data_ptr()),
        vp(loop._x0.data_ptr()), vp(loop._x_ref_win.data_ptr()), vp(loop._u_fb.data_ptr()),
        vp(loop._last_u.data_ptr()), vp(loop._have_last.data_ptr()), vp(loop._state.data_ptr()),
        vp(int(side.cuda_stream))), (loop,))
    assert args.launches + 3 <= loop._cap
    row = {"B": B}
    reset = lambda: loop.reset(x0)
    row["halfspaces_alone"] = timed(graph_of(halfspaces, side, dev), reset, B)
    row["solver_alone"] = timed(graph_of(solver, side, dev), reset, B)
    reset()
    row["advance_alone"] = timed(graph_of(advance, side, dev), reset, B)
    row["sum_ms"] = sum(row[k]["ms"] for k in ("halfspaces_alone", "solver_alone", "advance_alone"))
    return row


def main():
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_batch_times.py measures on the GPU; there is none")
    dev = torch.device("cuda", 0)
    parts = setup(dev)
    result = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "repeats": args.repeats,
              "launches": args.launches, "shape": {"O": 3, "H": H, "N": N, "P": P},
              "step_source_key": _native.source_key("drcvar_step.hip"),
              "timing": "device events around a window of back-to-back control steps, ms per control "
                        "step: median (min, max) over `repeats` windows; loop_steps_per_s = B / that"}
    result["single_graph_10_steps"] = single_row(dev, parts)
    print(json.dumps(result["single_graph_10_steps"]), flush=True)
    if args.part == "all":
        model, nominal, x_ref, u_ref, x0 = parts
        rows = []
        for B in BATCHES:
            row = {"B": B}
            for label, backend, per_graph in (("graph", "graph", 1), ("graph_10_steps", "graph", 10),
                                              ("launches", "launches", 1)):
                loop = closed_loop.RecedingHorizonBatch(model, nominal, x_ref, u_ref, N, RiskParams(),
                                                        n_problems=B, seed=SEED,
                                                        steps_per_graph=per_graph)
                row[label] = loop_windows(loop, starts(x0, B), backend, B)
            rows.append(row)
            print(json.dumps(row), flush=True)
        result["batch"] = rows
        result["single_graph_10_steps_again"] = single_row(dev, parts)
        result["launches_alone"] = launches_alone(dev, parts, BATCHES[-1])
        print(json.dumps(result["launches_alone"]), flush=True)
        ab = {"parent": [json.load(open(f))["single_graph_10_steps"] for f in args.ab_parent],
              "tree": [json.load(open(f))["single_graph_10_steps"] for f in args.ab_tree]}
        result["single_ab"] = ab
        singles = [result["single_graph_10_steps"], result["single_graph_10_steps_again"]] + ab["tree"]
        best_single = max(r["loop_steps_per_s_max"] for r in singles)
        result["batch_exceeds_single_beyond_the_spread"] = {
            str(r["B"]): bool(min(r[k]["loop_steps_per_s_min"] for k in ("graph", "graph_10_steps"))
                              > best_single) for r in rows if r["B"] in REQUIRED}
        if ab["parent"] and ab["tree"]:
            lo = min(r["ms_min"] for r in ab["parent"])
            hi = max(r["ms_max"] for r in ab["parent"])
            med = float(np.median([r["ms"] for r in ab["tree"]]))
            result["single_within_parent_spread"] = {
                "parent_ms_range": [lo, hi], "tree_ms_median": med, "holds": bool(lo <= med <= hi),
                "tree_faster_than_parent_range": bool(med < lo)}
    out = args.out or os.path.join(REPO, "profiles", "closed_loop", "closed_loop_batch_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
