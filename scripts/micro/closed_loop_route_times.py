"""Times the batched receding-horizon loop with a reference path per problem
(simulation/closed_loop.py, RecedingHorizonBatch with 3-D paths; the halfspace launch is
drcvar_sampled_halfspaces_f64_route, the advance drcvar_mpc_step_advance_batch_route_f64) and writes
profiles/closed_loop/closed_loop_route_times.json.

    python scripts/micro/closed_loop_route_times.py --part string [--tree DIR] --out FILE
    python scripts/micro/closed_loop_route_times.py [--out FILE] --ab-parent FILE ... --ab-tree FILE ...

Every timing but the use's is device-event time over a window of `--steps` back-to-back control
steps (or `--launches` launches) after a warm-up window: the median and the spread (min, max) of
`--repeats` windows.  Shape: main.py's (3 obstacles, H = 30, N = 20, P = 151), RecedingHorizonBatch
on `graph` with 10 steps per graph, problem b started from the scenario's start plus a small offset
of its own.

  --part string  only the 2-D batch (metric="dr_cvar", a RiskParams, one shared path; no new argument
                 is passed) at B = 1, 64 and 1024, importing the package from --tree: run on a build
                 of the parent commit and on this tree, alternated in one session (parent, tree,
                 parent, tree), and hand the files to the full run with --ab-parent / --ab-tree  (c)
  (full run)     (a) the halfspace launch alone in the metric form and in the route form, and the
                 advance alone in the batch form and in the route form, each replayed from a graph of
                 one launch, alternated; (b) per control step at the same B, alternated: the 2-D
                 string batch, the 2-D batch with B equal names (the metric launch: the route form's
                 solve and rows, on one shared path), B EQUAL routes given as 3-D paths (the route
                 launches on the same problems) and B DISTINCT routes (other problems); (d) one use:
                 4 candidate routes x 256 replicates with LoopEvaluation (M = 1000 Laplace
                 realisations, 100 steps) as ONE batch of 1024 loops against FOUR batches of 256: host
                 wall time of construction, capture, the run and safety(), end to end, with the
                 collision rate per route

Nothing here is a threshold: the file states whether the 2-D batch stayed within the parent's
spread, by how much the route launches differ from the forms they extend next to the run-to-run
spread, and the ratio of the two ways to compare the routes.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--part", choices=("all", "string"), default="all")
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
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core.mpc_filter import MPCModel  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import closed_loop  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import obstacles as ob  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.planner import (  # noqa: E402
    ReferenceTrajectoryPlanner)

SEED, H, N, P, DT = 5, 30, 20, 151, 0.2
BATCHES = (1, 64, 1024)
FORMS = ("string_2d", "equal_names_2d", "equal_routes", "distinct_routes")
# the use: four candidate routes from the scenario's start (goal, speed)
CANDIDATES = (((4.0, 0.0), 1.5), ((4.0, 1.0), 1.5), ((3.0, -1.0), 1.0), ((4.0, -1.0), 1.2))
REPLICATES, USE_M, USE_STEPS, LATERAL = 256, 1000, 100, 0.5


def spread(ms):
    ms = np.asarray(ms)
    return {"ms": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max())}


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
    return model, nominal, to(x_ref[:P]), to(u_ref[:P]), x0, cfg, planner


def starts(x0, B):
    offsets = 1e-2 * np.random.default_rng(11).standard_normal((B, 4))
    offsets[0] = 0.0
    return x0 + offsets


def distinct_routes(parts, B, dev):
    """B routes from the scenario's start: goals on a segment across the scenario's own goal, speeds
    between 1.0 and 1.5 (problem 0: the scenario's own route)."""
    cfg, planner = parts[5], parts[6]
    goal = np.asarray(cfg["ego_goal"], dtype=np.float64)
    goals = np.tile(goal, (B, 1))
    goals[:, 1] += np.linspace(0.0, 1.0, B) * np.where(np.arange(B) % 2 == 0, 1.0, -1.0)
    speeds = 1.5 - 0.5 * (np.arange(B) % 5) / 4.0
    x_ref, u_ref = planner.straight_line_routes(cfg["ego_start"], goals, speeds)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return to(x_ref[:, :P]), to(u_ref[:, :P])


def batch(parts, B, form, dev=None, **kw):
    model, nominal, x_ref, u_ref = parts[:4]
    if form == "string_2d":        # (what the parent commit's build is given too)
        kw.setdefault("metric", "dr_cvar")
    elif form == "equal_names_2d":
        kw.setdefault("metric", ["dr_cvar"] * B)
    elif form == "equal_routes":
        x_ref, u_ref = x_ref[None].expand(B, -1, -1), u_ref[None].expand(B, -1, -1)
    elif "paths" in kw:
        x_ref, u_ref = kw.pop("paths")
    else:
        x_ref, u_ref = distinct_routes(parts, B, dev)
    return closed_loop.RecedingHorizonBatch(model, nominal, x_ref, u_ref, N, RiskParams(), n_problems=B,
                                            seed=SEED, steps_per_graph=10, **kw)


def loop_windows(loop, x0):
    """ms per control step of `--repeats` windows of `--steps` steps, each from a reset."""
    result = []
    loop.reset(x0)
    result[:] = loop.run(args.steps, backend="graph")        # captures / warms up
    ms = []
    for _ in range(args.repeats):
        loop.reset(x0)                                       # same first step: the capture is kept
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        result[:] = loop.run(args.steps, backend="graph")
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / args.steps)
    row = spread(ms)
    status = result[2][..., 0]
    row["solved_share"] = float(((status == 0) | (status == 3)).double().mean())
    row["mean_iterations"] = float(result[2][..., 1].mean())
    return row


def graph_of(launch, side):
    """A graph of the one launch `launch` issues on `side` (run once eagerly first)."""
    with torch.cuda.stream(side):
        launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch()
    return graph.replay


def timed(fn):
    """ms per call of fn: windows of `--launches` back-to-back calls between two device events."""
    for _ in range(3):
        fn()
    ms = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / args.launches)
    return spread(ms)


def advance_launch(loop, side, route):
    """The advance of `loop` (after a run: logs exist) as one prepared launch on `side`, in the
    batch form or, on the same buffers with each problem's own path strides, in the route form."""
    m, vp = loop.model, ctypes.c_void_p
    x_log, u_log, info_log = loop._logs
    if route:
        entry = _native.route_lib().drcvar_mpc_step_advance_batch_route_f64
        strides = (loop.x_ref_path.stride(0), loop.u_ref_path.stride(0))
    else:
        entry, strides = _native.loop_lib().drcvar_mpc_step_advance_batch_f64, ()
    return engine.PreparedLaunch(entry, (
        ctypes.pointer(m.model), loop.n_problems, vp(loop._x.data_ptr()), vp(loop._u.data_ptr()),
        vp(loop._info.data_ptr()), vp(loop.x_ref_path.data_ptr()), vp(loop.u_ref_path.data_ptr()),
        loop.path_steps, *strides, vp(None), loop._step_begin, loop._cap, vp(x_log.data_ptr()),
        vp(u_log.data_ptr()), vp(info_log.data_ptr()), vp(loop._x0.data_ptr()),
        vp(loop._x_ref_win.data_ptr()), vp(loop._u_fb.data_ptr()), vp(loop._last_u.data_ptr()),
        vp(loop._have_last.data_ptr()), vp(loop._state.data_ptr()), vp(int(side.cuda_stream))),
        (loop, x_log, u_log, info_log))


def launches_alone(dev, parts, B):
    """(a) The halfspace launch of one control step alone at B problems in the metric form (one
    shared path), in the route form (B distinct routes) and in the route form with problem stride 0
    (problem 0's route for all), and the advance alone in the batch form
    and in the route form (the route loop's buffers; the batch form reads problem 0's paths), from
    the buffers of a loop that has run one graph."""
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    loop = batch(parts, B, "distinct_routes", dev)
    loop.reset(starts(parts[4], B))
    loop.run(10, backend="graph")
    torch.cuda.synchronize()
    common = dict(draw_period=B, table=loop._risk_table, codes=loop._codes, seed=SEED, out=loop._record,
                  selected=loop._selected, stream=side)
    metric, _, _ = engine.prepare_sampled_halfspaces_metric(
        loop.nominal_path, loop.ego_path[0], loop.n_obstacles, H, N, loop.params, loop.metrics,
        loop._state[0], **common)
    route, _, _ = engine.prepare_sampled_halfspaces_route(
        loop.nominal_path, loop.ego_path, loop.n_obstacles, H, N, loop.params, loop.metrics,
        loop._state[0], **common)
    # (the route form on ONE path, problem stride 0: the form's instructions without its B paths'
    # addresses, which tells the address chain from the scalar cache's misses)
    shared, _, _ = engine.prepare_sampled_halfspaces_route(
        loop.nominal_path, loop.ego_path[:1].expand(B, -1, -1), loop.n_obstacles, H, N, loop.params,
        loop.metrics, loop._state[0], **common)
    replays = {"metric_form": graph_of(metric, side), "route_form": graph_of(route, side),
               "route_form_stride_0": graph_of(shared, side),
               "batch_advance": graph_of(advance_launch(loop, side, False), side),
               "route_advance": graph_of(advance_launch(loop, side, True), side)}
    row = {"B": B}
    for _ in range(3):                       # alternated
        for name, replay in replays.items():
            row.setdefault(name, []).append(timed(replay))
    med = {name: float(np.median([r["ms"] for r in row[name]])) for name in replays}
    width = {name: max(r["ms_max"] for r in row[name]) - min(r["ms_min"] for r in row[name])
             for name in replays}
    row["route_minus_metric_us"] = 1e3 * (med["route_form"] - med["metric_form"])
    row["route_stride_0_minus_metric_us"] = 1e3 * (med["route_form_stride_0"] - med["metric_form"])
    row["halfspace_spread_us"] = 1e3 * max(width["route_form"], width["metric_form"])
    row["route_advance_minus_batch_us"] = 1e3 * (med["route_advance"] - med["batch_advance"])
    row["advance_spread_us"] = 1e3 * max(width["route_advance"], width["batch_advance"])
    return row


def use(dev, parts):
    """(d) Four candidate routes x 256 replicates (laterally spread starts), 100 evaluated steps:
    once as ONE batch of 1024 loops (problem b = route 256 + replicate, draw_period = 256: every
    route meets the same replicate draws), once as FOUR batches of 256 loops with one shared 2-D
    path each.  Host wall time around construction, capture, the run and safety(), ending in a
    synchronise."""
    x0, cfg, planner = parts[4], parts[5], parts[6]
    along = np.asarray(cfg["ego_goal"], dtype=np.float64) - np.asarray(cfg["ego_start"], dtype=np.float64)
    across = np.array([-along[1], along[0]]) / np.linalg.norm(along)
    x0r = np.tile(x0, (REPLICATES, 1))
    x0r[:, :2] += np.linspace(-LATERAL, LATERAL, REPLICATES)[:, None] * across
    goals = np.array([g for g, _ in CANDIDATES])
    speeds = np.array([v for _, v in CANDIDATES])
    x4, u4 = planner.straight_line_routes(cfg["ego_start"], goals, speeds)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x4, u4 = to(x4[:, :P]), to(u4[:, :P])
    R = len(CANDIDATES)
    p = RiskParams()
    evaluate = closed_loop.LoopEvaluation(USE_M, noise="laplace", robot_radius=p.robot_radius,
                                          obstacle_radius=p.obstacle_radius, seed=77,
                                          independent_problems=False)

    def one_batch():
        paths = (x4.repeat_interleave(REPLICATES, dim=0), u4.repeat_interleave(REPLICATES, dim=0))
        loop = batch(parts, R * REPLICATES, "distinct_routes", paths=paths, draw_period=REPLICATES,
                     evaluate=evaluate)
        loop.reset(np.tile(x0r, (R, 1)))
        result = loop.run(USE_STEPS, backend="graph")
        s = loop.safety()
        return result[1].cpu(), s["min_clearance"].cpu(), s["collided"].cpu(), result[2][..., 0].cpu()

    def four_batches():
        parts_out = [[], [], [], []]
        for r in range(R):
            one = parts[:2] + (x4[r].contiguous(), u4[r].contiguous()) + parts[4:]
            loop = batch(one, REPLICATES, "string_2d", evaluate=evaluate)
            loop.reset(x0r)
            result = loop.run(USE_STEPS, backend="graph")
            s = loop.safety()
            for acc, t in zip(parts_out, (result[1], s["min_clearance"], s["collided"], result[2][..., 0])):
                acc.append(t.cpu())
        return tuple(torch.cat(acc) for acc in parts_out)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    one_batch(), four_batches()                  # warm-up: code objects, allocator, both paths once
    seconds = {"one_batch": [], "four_batches": []}
    for _ in range(5):                            # alternated
        one, t = wall(one_batch)
        seconds["one_batch"].append(t)
        four, t = wall(four_batches)
        seconds["four_batches"].append(t)
    same = all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(one, four))
    clearance, collided = one[1].view(R, REPLICATES, USE_M), one[2].view(R, REPLICATES)
    solved = ((one[3] == 0) | (one[3] == 3)).double().view(R, -1)
    table = [{"goal": list(CANDIDATES[r][0]), "speed": CANDIDATES[r][1],
              "collision_rate": float(collided[r].mean()),
              "collision_rate_four_batches": float(four[2].view(R, REPLICATES)[r].mean()),
              "loops_with_a_collision": int((collided[r] > 0).sum()),
              "solved_share": float(solved[r].mean()),
              "mean_min_clearance": float(clearance[r].mean()),
              "min_min_clearance": float(clearance[r].min())} for r in range(R)]
    med = {k: float(np.median(v)) for k, v in seconds.items()}
    ranges = {k: [min(v), max(v)] for k, v in seconds.items()}
    return {"routes": R, "replicates": REPLICATES, "B": R * REPLICATES, "M": USE_M, "steps": USE_STEPS,
            "lateral_spread_m": LATERAL, "wall_seconds": seconds, "wall_seconds_median": med,
            "wall_seconds_range": ranges, "four_over_one": med["four_batches"] / med["one_batch"],
            "one_batch_faster_beyond_the_spread": bool(ranges["one_batch"][1] < ranges["four_batches"][0]),
            "results_bitwise_equal": bool(same),
            # (the solver's workgroup size depends on B, so a problem of the batch of 1024 need not be
            # bitwise the problem of a batch of 256: the differences, where there are any)
            "max_abs_input_difference": float((one[0] - four[0]).abs().max()),
            "max_abs_collision_rate_difference": float((one[2] - four[2]).abs().max()),
            "per_route": table}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_route_times.py measures on the GPU; there is none")
    dev = torch.device("cuda", 0)
    parts = setup(dev)
    result = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "repeats": args.repeats,
              "launches": args.launches, "shape": {"O": 3, "H": H, "N": N, "P": P},
              "sampled_source_key": _native.source_key("drcvar_sampled.hip"),
              "step_source_key": _native.source_key("drcvar_step.hip"),
              "timing": "device events around a window of back-to-back control steps (graph, 10 steps "
                        "per graph), ms per control step: median (min, max) over `repeats` windows"}
    forms = ("string_2d",) if args.part == "string" else FORMS
    rows = []
    for B in BATCHES:
        row = {"B": B}
        for _ in range(1 if args.part == "string" else 2):     # alternated within the session
            for form in forms:
                row.setdefault(form, []).append(loop_windows(batch(parts, B, form, dev), starts(parts[4], B)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    result["batch"] = rows
    if args.part == "all":
        result["launches_alone"] = [launches_alone(dev, parts, B) for B in BATCHES]
        print(json.dumps(result["launches_alone"]), flush=True)
        result["use"] = use(dev, parts)
        print(json.dumps(result["use"]), flush=True)
        ab = {"parent": [json.load(open(f))["batch"] for f in args.ab_parent],
              "tree": [json.load(open(f))["batch"] for f in args.ab_tree]}
        result["string_ab"] = ab
        summary = {}
        for k, B in enumerate(BATCHES):
            med = {f: float(np.median([r["ms"] for r in rows[k][f]])) for f in FORMS}
            rng = {f: [min(r["ms_min"] for r in rows[k][f]), max(r["ms_max"] for r in rows[k][f])] for f in FORMS}
            entry = {"ms_median": med, "ms_range": rng,
                     "equal_routes_minus_equal_names_us": 1e3 * (med["equal_routes"] - med["equal_names_2d"]),
                     "equal_routes_slower_beyond_the_spread":
                         bool(rng["equal_routes"][0] > rng["equal_names_2d"][1]),
                     "distinct_minus_equal_routes_us": 1e3 * (med["distinct_routes"] - med["equal_routes"]),
                     "mean_iterations": {f: rows[k][f][0]["mean_iterations"] for f in FORMS}}
            if ab["parent"] and ab["tree"]:
                par = [run[k]["string_2d"][0] for run in ab["parent"]]
                tre = [run[k]["string_2d"][0] for run in ab["tree"]] + rows[k]["string_2d"]
                lo, hi = min(r["ms_min"] for r in par), max(r["ms_max"] for r in par)
                t_lo, t_hi = min(r["ms_min"] for r in tre), max(r["ms_max"] for r in tre)
                entry["parent_string_ms_range"] = [lo, hi]
                entry["tree_string_ms_range"] = [t_lo, t_hi]
                entry["parent_string_ms_median"] = float(np.median([r["ms"] for r in par]))
                entry["tree_string_ms_median"] = float(np.median([r["ms"] for r in tre]))
                entry["string_ranges_overlap"] = bool(t_lo <= hi and lo <= t_hi)
            summary[str(B)] = entry
        result["summary"] = summary
        print(json.dumps(summary), flush=True)
    out = args.out or os.path.join(REPO, "profiles", "closed_loop", "closed_loop_route_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
