"""Times the batched receding-horizon loop with a metric per problem (simulation/closed_loop.py,
RecedingHorizonBatch(metric=[...]); the halfspace launch is drcvar_sampled_halfspaces_f64_metric)
and writes profiles/closed_loop/closed_loop_metric_times.json.

    python scripts/micro/closed_loop_metric_times.py --part string [--tree DIR] --out FILE
    python scripts/micro/closed_loop_metric_times.py [--out FILE] --ab-parent FILE ... --ab-tree FILE ...

Every timing but the comparison's is device-event time over a window of `--steps` back-to-back
control steps (or `--launches` launches) after a warm-up window: the median and the spread (min,
max) of `--repeats` windows.  Shape: main.py's (3 obstacles, H = 30, N = 20, P = 151),
RecedingHorizonBatch on `graph` with 10 steps per graph, problem b started from the scenario's start
plus a small offset of its own.

  --part string  only the string-metric path (metric="dr_cvar", a RiskParams; no new argument is
                 passed) at B = 1, 64 and 1024, importing the package from --tree: run on a build of
                 the parent commit and on this tree, alternated in one session (parent, tree, parent,
                 tree), and hand the files to the full run with --ab-parent / --ab-tree
  (full run)     the string path, a sequence of B times "dr_cvar" (the new launch and the solve on
                 its rows, on the string path's own problems) and the mixed batch (metrics cycling
                 mean, cvar, dr_cvar: other problems, with other iteration counts) per control step
                 at the same B, alternated; the halfspace launch alone in the
                 risk-table form and in the metric form, each replayed from a graph of one launch,
                 alternated; then the comparison: the three metrics x D = 341 replicates on common
                 random numbers as ONE batch of 1023 loops against THREE batches of 341 (each with
                 LoopEvaluation, M = 1000 Laplace realisations shared by all problems, 100 steps):
                 host wall time of construction, capture, the run and safety(), end to end

Nothing here is a threshold: the file states whether the string path stayed within the parent's
spread, by how much the metric launch differs from the risk-table launch in the same session, and
the ratio of the two ways to compare the metrics.
"""
import argparse
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
NAMES = ("mean", "cvar", "dr_cvar")
FORMS = ("string", "equal_names", "mixed")
REPLICATES, CMP_M, CMP_STEPS, LATERAL = 341, 1000, 100, 1.0


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
    return model, nominal, to(x_ref[:P]), to(u_ref[:P]), x0, cfg


def starts(x0, B):
    offsets = 1e-2 * np.random.default_rng(11).standard_normal((B, 4))
    offsets[0] = 0.0
    return x0 + offsets


def batch(parts, B, form, **kw):
    model, nominal, x_ref, u_ref = parts[:4]
    if form == "string":        # (what the parent commit's build is given too)
        kw.setdefault("metric", "dr_cvar")
    elif form == "equal_names":   # the new path on the string path's problems: the path's own cost
        kw.setdefault("metric", ["dr_cvar"] * B)
    else:                         # (mean and CVaR problems take more interior-point iterations)
        kw.setdefault("metric", [NAMES[b % 3] for b in range(B)])
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


def halfspaces_alone(dev, parts, B):
    """The halfspace launch of one control step alone at B problems, in the risk-table form and in
    the metric form (the same table of equal rows, D = B, metrics cycling), from the first step's
    buffers."""
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    loop = batch(parts, B, "mixed")
    loop.reset(starts(parts[4], B))
    common = dict(draw_period=B, table=loop._risk_table, seed=SEED, out=loop._record, stream=side)
    risk, _ = engine.prepare_sampled_halfspaces_risk(
        loop.nominal_path, loop.ego_path, loop.n_obstacles, H, N, loop.params, loop._state[0], **common)
    metric, _, _ = engine.prepare_sampled_halfspaces_metric(
        loop.nominal_path, loop.ego_path, loop.n_obstacles, H, N, loop.params, loop.metrics,
        loop._state[0], codes=loop._codes, selected=loop._selected, **common)
    replays = {"risk_form": graph_of(risk, side), "metric_form": graph_of(metric, side)}
    row = {"B": B}
    for _ in range(3):                       # alternated: risk, metric, risk, metric, risk, metric
        for name, replay in replays.items():
            row.setdefault(name, []).append(timed(replay))
    med = {name: float(np.median([r["ms"] for r in row[name]])) for name in replays}
    row["metric_over_risk"] = med["metric_form"] / med["risk_form"]
    row["metric_minus_risk_us"] = 1e3 * (med["metric_form"] - med["risk_form"])
    return row


def comparison(dev, parts):
    """mean, CVaR and DR-CVaR x 341 replicates (laterally spread starts), 100 evaluated steps on
    common random numbers: once as ONE batch of 1023 loops (metric per problem, draw_period = 341,
    problem b = s 341 + r), once as THREE batches of 341 loops with one metric each.  Host wall
    time around construction, capture, the run and safety(), ending in a synchronise."""
    model, nominal, x_ref, u_ref, x0, cfg = parts
    along = np.asarray(cfg["ego_goal"], dtype=np.float64) - np.asarray(cfg["ego_start"], dtype=np.float64)
    across = np.array([-along[1], along[0]]) / np.linalg.norm(along)
    x0r = np.tile(x0, (REPLICATES, 1))
    x0r[:, :2] += np.linspace(-LATERAL, LATERAL, REPLICATES)[:, None] * across
    p = RiskParams()
    evaluate = closed_loop.LoopEvaluation(CMP_M, noise="laplace", robot_radius=p.robot_radius,
                                          obstacle_radius=p.obstacle_radius, seed=77,
                                          independent_problems=False)

    def one_batch():
        loop = batch(parts, 3 * REPLICATES, "mixed", metric=[m for m in NAMES for _ in range(REPLICATES)],
                     draw_period=REPLICATES, evaluate=evaluate)
        loop.reset(np.tile(x0r, (3, 1)))
        result = loop.run(CMP_STEPS, backend="graph")
        s = loop.safety()
        return result[1].cpu(), s["min_clearance"].cpu(), s["collided"].cpu(), result[2][..., 0].cpu()

    def three_batches():
        parts_out = [[], [], [], []]
        for name in NAMES:
            loop = batch(parts, REPLICATES, "string", metric=name, evaluate=evaluate)
            loop.reset(x0r)
            result = loop.run(CMP_STEPS, backend="graph")
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

    one_batch(), three_batches()                 # warm-up: code objects, allocator, both paths once
    seconds = {"one_batch": [], "three_batches": []}
    for _ in range(5):                            # alternated
        one, t = wall(one_batch)
        seconds["one_batch"].append(t)
        three, t = wall(three_batches)
        seconds["three_batches"].append(t)
    same = all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(one, three))
    clearance, collided = one[1].view(3, REPLICATES, CMP_M), one[2].view(3, REPLICATES)
    solved = ((one[3] == 0) | (one[3] == 3)).double().view(3, -1)
    table = [{"metric": name, "collision_rate": float(collided[s].mean()),
              "loops_with_a_collision": int((collided[s] > 0).sum()),
              "solved_share": float(solved[s].mean()),
              "mean_min_clearance": float(clearance[s].mean()),
              "min_min_clearance": float(clearance[s].min())} for s, name in enumerate(NAMES)]
    med = {k: float(np.median(v)) for k, v in seconds.items()}
    ranges = {k: [min(v), max(v)] for k, v in seconds.items()}
    return {"metrics": list(NAMES), "replicates": REPLICATES, "B": 3 * REPLICATES, "M": CMP_M,
            "steps": CMP_STEPS, "lateral_spread_m": LATERAL, "wall_seconds": seconds,
            "wall_seconds_median": med, "wall_seconds_range": ranges,
            "three_over_one": med["three_batches"] / med["one_batch"],
            "one_batch_faster_beyond_the_spread": bool(ranges["one_batch"][1] < ranges["three_batches"][0]),
            "results_bitwise_equal": bool(same),
            # (the solver's workgroup size depends on B, so a problem of the batch of 1023 need not be
            # bitwise the problem of a batch of 341: the differences, where there are any)
            "max_abs_input_difference": float((one[0] - three[0]).abs().max()),
            "max_abs_collision_rate_difference": float((one[2] - three[2]).abs().max()),
            "per_metric": table}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_metric_times.py measures on the GPU; there is none")
    dev = torch.device("cuda", 0)
    parts = setup(dev)
    result = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "repeats": args.repeats,
              "launches": args.launches, "shape": {"O": 3, "H": H, "N": N, "P": P},
              "sampled_source_key": _native.source_key("drcvar_sampled.hip"),
              "timing": "device events around a window of back-to-back control steps (graph, 10 steps "
                        "per graph), ms per control step: median (min, max) over `repeats` windows"}
    forms = ("string",) if args.part == "string" else FORMS
    rows = []
    for B in BATCHES:
        row = {"B": B}
        for _ in range(1 if args.part == "string" else 2):     # alternated within the session
            for form in forms:
                row.setdefault(form, []).append(loop_windows(batch(parts, B, form), starts(parts[4], B)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    result["batch"] = rows
    if args.part == "all":
        result["halfspaces_alone"] = [halfspaces_alone(dev, parts, B) for B in BATCHES]
        print(json.dumps(result["halfspaces_alone"]), flush=True)
        result["comparison"] = comparison(dev, parts)
        print(json.dumps(result["comparison"]), flush=True)
        ab = {"parent": [json.load(open(f))["batch"] for f in args.ab_parent],
              "tree": [json.load(open(f))["batch"] for f in args.ab_tree]}
        result["string_ab"] = ab
        summary = {}
        for k, B in enumerate(BATCHES):
            ref = rows[k]["string"]
            ref_med = float(np.median([r["ms"] for r in ref]))
            mixed = float(np.median([r["ms"] for r in rows[k]["mixed"]]))
            equal = float(np.median([r["ms"] for r in rows[k]["equal_names"]]))
            entry = {"string_ms_median": ref_med, "equal_names_ms_median": equal, "mixed_ms_median": mixed,
                     "string_ms_range": [min(r["ms_min"] for r in ref), max(r["ms_max"] for r in ref)],
                     "equal_names_minus_string_us": 1e3 * (equal - ref_med),
                     "mixed_minus_string_us": 1e3 * (mixed - ref_med),
                     "mean_iterations": {f: rows[k][f][0]["mean_iterations"] for f in FORMS}}
            if ab["parent"] and ab["tree"]:
                par = [run[k]["string"][0] for run in ab["parent"]]
                tre = [run[k]["string"][0] for run in ab["tree"]] + ref
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
    out = args.out or os.path.join(REPO, "profiles", "closed_loop", "closed_loop_metric_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
