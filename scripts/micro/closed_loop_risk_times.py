"""Times the batched receding-horizon loop with risk parameters per problem
(simulation/closed_loop.py, RecedingHorizonBatch(params=RiskTable(...), draw_period=D); the
halfspace launch is drcvar_sampled_halfspaces_f64_risk) against the batch with one RiskParams,
measures what a one-batch sweep over (epsilon, alpha) buys, and writes
profiles/closed_loop/closed_loop_risk_times.json.

    python scripts/micro/closed_loop_risk_times.py --part reference [--tree DIR] --out FILE
    python scripts/micro/closed_loop_risk_times.py [--out FILE] --ab-parent FILE ... --ab-tree FILE ...

Every timing but the sweep's is device-event time over a window of `--steps` back-to-back control
steps after a warm-up window: the median and the spread (min, max) of `--repeats` windows, in ms
per control step.  Shape: main.py's (3 obstacles, H = 30, N = 20, P = 151), RecedingHorizonBatch on
`graph` with 10 steps per graph, problem b started from the scenario's start plus a small offset of
its own.

  --part reference  only params=RiskParams (no new argument is passed) at B = 1, 64 and 1024,
                    importing the package from --tree: run on a build of the parent commit and on
                    this tree, alternated in one session (parent, tree, parent, tree), and hand the
                    files to the full run with --ab-parent / --ab-tree
  (full run)        per control step: RiskParams, a RiskTable with D = B and with D = 1, at the same
                    B, alternated; the halfspace launch alone in the device-state form, the
                    risk-table form (D = B, D = 1) and the predicted-ego form, replayed from a graph
                    of one launch; then the sweep: a 5 x 4 grid of (epsilon, alpha) x 50 replicates
                    as ONE batch of 1000 loops against the same 20 settings as 20 batches of 50
                    loops (LoopEvaluation, M = 1000 Laplace realisations shared by all problems, 100
                    steps), host wall time end to end, with the table of collision rate and mean
                    minimum clearance per setting

Nothing here is a threshold: the file states whether RiskParams stayed within the parent's spread
and by how much the table form differs from the device-state form in the same session.
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
ap.add_argument("--part", choices=("all", "reference"), default="all")
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
FORMS = ("params", "table_full_period", "table_period_1")
EPSILONS, ALPHAS, DELTA = (0.0, 0.05, 0.15, 0.3, 0.6), (0.05, 0.1, 0.2, 0.4), 0.1
REPLICATES, SWEEP_M, SWEEP_STEPS, LATERAL = 50, 1000, 100, 1.0


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


def equal_rows(B):
    p = RiskParams()
    return engine.RiskTable(alpha=[p.alpha] * B, delta=p.delta, epsilon=p.epsilon,
                            robot_radius=p.robot_radius, obstacle_radius=p.obstacle_radius)


def batch(parts, B, form, params=None, **kw):
    model, nominal, x_ref, u_ref = parts[:4]
    if form == "params":        # (what the parent commit's build is given too)
        params = RiskParams() if params is None else params
    else:
        params = equal_rows(B) if params is None else params
        kw.setdefault("draw_period", 1 if form == "table_period_1" else None)
    return closed_loop.RecedingHorizonBatch(model, nominal, x_ref, u_ref, N, params, n_problems=B,
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
    """The halfspace launch of one control step alone at B problems, in the device-state form, the
    risk-table form (D = B and D = 1) and the predicted-ego form, from the first step's buffers (the
    launch writes the record and nothing else)."""
    x0 = starts(parts[4], B)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    row = {"B": B}
    loop = batch(parts, B, "params")
    loop.reset(x0)
    common = dict(seed=SEED, out=loop._record, stream=side)
    dev_form, _ = engine.prepare_sampled_halfspaces_dev(
        loop.nominal_path, loop.ego_path, H, N, RiskParams(), loop._state[0], **common)
    table = equal_rows(B)
    rows = table.to_device(N, dev)
    risk = {D: engine.prepare_sampled_halfspaces_risk(
        loop.nominal_path, loop.ego_path, loop.n_obstacles, H, N, table, loop._state[0], draw_period=D,
        table=rows, **common)[0] for D in (B, 1)}
    loop_p = batch(parts, B, "params", linearize="predicted")
    loop_p.reset(x0)
    replays = {"dev_form": graph_of(dev_form, side),
               "risk_form_full_period": graph_of(risk[B], side),
               "risk_form_period_1": graph_of(risk[1], side),
               "pred_form_shift_1": graph_of(loop_p._lin_launch(side, 1), side)}
    for _ in range(2):                       # alternated: dev, risk, risk, pred, dev, risk, risk, pred
        for name, replay in replays.items():
            row.setdefault(name, []).append(timed(replay))
    med = {name: float(np.median([r["ms"] for r in runs])) for name, runs in row.items() if name != "B"}
    row["over_dev_form"] = {name: v / med["dev_form"] for name, v in med.items() if name != "dev_form"}
    return row


def sweep(dev, parts):
    """The 5 x 4 grid of (epsilon, alpha) x 50 replicates, 100 evaluated steps: once as one batch of
    1000 loops on a RiskTable with draw_period = 50 (problem b = s 50 + r), once as 20 batches of 50
    loops with one RiskParams each.  Both see the same draws, starts and realisations, so the
    results must be the same bits; the wall time (host clock around construction, capture, the run
    and safety(), ending in a synchronise) is what differs."""
    model, nominal, x_ref, u_ref, x0, cfg = parts
    along = np.asarray(cfg["ego_goal"], dtype=np.float64) - np.asarray(cfg["ego_start"], dtype=np.float64)
    across = np.array([-along[1], along[0]]) / np.linalg.norm(along)
    x0r = np.tile(x0, (REPLICATES, 1))
    x0r[:, :2] += np.linspace(-LATERAL, LATERAL, REPLICATES)[:, None] * across
    settings = [(e, a) for e in EPSILONS for a in ALPHAS]
    S = len(settings)
    p = RiskParams()
    evaluate = closed_loop.LoopEvaluation(SWEEP_M, noise="laplace", robot_radius=p.robot_radius,
                                          obstacle_radius=p.obstacle_radius, seed=77,
                                          independent_problems=False)

    def one_batch():
        table = engine.RiskTable(alpha=np.repeat([a for _, a in settings], REPLICATES), delta=DELTA,
                                 epsilon=np.repeat([e for e, _ in settings], REPLICATES),
                                 robot_radius=p.robot_radius, obstacle_radius=p.obstacle_radius)
        loop = batch(parts, S * REPLICATES, "table", params=table, draw_period=REPLICATES, evaluate=evaluate)
        loop.reset(np.tile(x0r, (S, 1)))
        result = loop.run(SWEEP_STEPS, backend="graph")
        s = loop.safety()
        return result[1].cpu(), s["min_clearance"].cpu(), s["collided"].cpu(), result[2][..., 0].cpu()

    def twenty_batches():
        inputs, clearance, collided, status = [], [], [], []
        for e, a in settings:
            params = RiskParams(p.robot_radius, p.obstacle_radius, a, DELTA, e)
            loop = batch(parts, REPLICATES, "params", params=params, evaluate=evaluate)
            loop.reset(x0r)
            result = loop.run(SWEEP_STEPS, backend="graph")
            s = loop.safety()
            inputs.append(result[1].cpu())
            clearance.append(s["min_clearance"].cpu())
            collided.append(s["collided"].cpu())
            status.append(result[2][..., 0].cpu())
        return torch.cat(inputs), torch.cat(clearance), torch.cat(collided), torch.cat(status)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    one_batch(), twenty_batches()                # warm-up: code objects, allocator, both paths once
    seconds = {"one_batch": [], "twenty_batches": []}
    for _ in range(3):                            # alternated
        one, t = wall(one_batch)
        seconds["one_batch"].append(t)
        twenty, t = wall(twenty_batches)
        seconds["twenty_batches"].append(t)
    same = all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(one, twenty))
    clearance, collided = one[1].view(S, REPLICATES, SWEEP_M), one[2].view(S, REPLICATES)
    solved = ((one[3] == 0) | (one[3] == 3)).double().view(S, -1)
    table = [{"epsilon": e, "alpha": a, "collision_rate": float(collided[s].mean()),
              "loops_with_a_collision": int((collided[s] > 0).sum()),
              "solved_share": float(solved[s].mean()),
              "mean_min_clearance": float(clearance[s].mean()),
              "min_min_clearance": float(clearance[s].min())} for s, (e, a) in enumerate(settings)]
    med = {k: float(np.median(v)) for k, v in seconds.items()}
    return {"settings": S, "replicates": REPLICATES, "B": S * REPLICATES, "M": SWEEP_M,
            "steps": SWEEP_STEPS, "delta": DELTA, "lateral_spread_m": LATERAL,
            "wall_seconds": seconds, "wall_seconds_median": med,
            "twenty_over_one": med["twenty_batches"] / med["one_batch"],
            "results_bitwise_equal": bool(same),
            # (the solver's workgroup size depends on B, so a problem of the batch of 1000 need not
            # be bitwise the problem of a batch of 50: the differences, where there are any)
            "max_abs_input_difference": float((one[0] - twenty[0]).abs().max()),
            "max_abs_collision_rate_difference": float((one[2] - twenty[2]).abs().max()),
            "per_setting": table}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_risk_times.py measures on the GPU; there is none")
    dev = torch.device("cuda", 0)
    parts = setup(dev)
    result = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "repeats": args.repeats,
              "launches": args.launches, "shape": {"O": 3, "H": H, "N": N, "P": P},
              "sampled_source_key": _native.source_key("drcvar_sampled.hip"),
              "timing": "device events around a window of back-to-back control steps (graph, 10 steps "
                        "per graph), ms per control step: median (min, max) over `repeats` windows"}
    forms = ("params",) if args.part == "reference" else FORMS
    rows = []
    for B in BATCHES:
        row = {"B": B}
        for _ in range(1 if args.part == "reference" else 2):     # alternated within the session
            for form in forms:
                row.setdefault(form, []).append(loop_windows(batch(parts, B, form), starts(parts[4], B)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    result["batch"] = rows
    if args.part == "all":
        result["halfspaces_alone"] = [halfspaces_alone(dev, parts, B) for B in BATCHES]
        print(json.dumps(result["halfspaces_alone"]), flush=True)
        result["sweep"] = sweep(dev, parts)
        print(json.dumps(result["sweep"]), flush=True)
        ab = {"parent": [json.load(open(f))["batch"] for f in args.ab_parent],
              "tree": [json.load(open(f))["batch"] for f in args.ab_tree]}
        result["params_ab"] = ab
        summary = {}
        for k, B in enumerate(BATCHES):
            ref = rows[k]["params"]
            ref_lo, ref_hi = min(r["ms_min"] for r in ref), max(r["ms_max"] for r in ref)
            ref_med = float(np.median([r["ms"] for r in ref]))
            entry = {"params_ms_range": [ref_lo, ref_hi], "params_ms_median": ref_med}
            for form in FORMS[1:]:
                med = float(np.median([r["ms"] for r in rows[k][form]]))
                entry[form + "_ms_median"] = med
                entry[form + "_minus_params_us"] = 1e3 * (med - ref_med)
                entry[form + "_within_params_range"] = bool(ref_lo <= med <= ref_hi)
            if ab["parent"] and ab["tree"]:
                par = [run[k]["params"][0] for run in ab["parent"]]
                tre = [run[k]["params"][0] for run in ab["tree"]] + ref
                lo, hi = min(r["ms_min"] for r in par), max(r["ms_max"] for r in par)
                t_lo, t_hi = min(r["ms_min"] for r in tre), max(r["ms_max"] for r in tre)
                entry["parent_params_ms_range"] = [lo, hi]
                entry["tree_params_ms_range"] = [t_lo, t_hi]
                entry["params_ranges_overlap"] = bool(t_lo <= hi and lo <= t_hi)
            summary[str(B)] = entry
        result["summary"] = summary
        print(json.dumps(summary), flush=True)
    out = args.out or os.path.join(REPO, "profiles", "closed_loop", "closed_loop_risk_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
