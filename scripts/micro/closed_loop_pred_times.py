"""Times the receding-horizon loops linearised about their own predicted path
(simulation/closed_loop.py, linearize="predicted", relinearize=r) against the loops linearised
about the reference path, measures what the predicted linearisation buys in closed-loop safety, and
writes profiles/closed_loop/closed_loop_pred_times.json.

    python scripts/micro/closed_loop_pred_times.py --part reference [--tree DIR] --out FILE
    python scripts/micro/closed_loop_pred_times.py [--out FILE] --ab-parent FILE ... --ab-tree FILE ...

Every timing is device-event time over a window of `--steps` back-to-back control steps after a
warm-up window: the median and the spread (min, max) of `--repeats` windows, in ms per control
step.  Shape: main.py's (3 obstacles, H = 30, N = 20, P = 151), RecedingHorizonBatch on `graph`
with 10 steps per graph, problem b started from the scenario's start plus a small offset of its own.

  --part reference  only linearize="reference" (the default: no new argument is passed) at B = 1,
                    64 and 1024, importing the package from --tree: run on a build of the parent
                    commit and on this tree, alternated in one session (parent, tree, parent,
                    tree), and hand the files to the full run with --ab-parent / --ab-tree
  (full run)        "reference", "predicted" and "predicted" with relinearize=1 at the same B,
                    alternated; at B = 1024 the halfspace launch alone in both forms, replayed from
                    a graph of one launch; then the closed-loop safety of the three at B = 1024
                    starts spread laterally about the scenario's start (LoopEvaluation, M = 1000
                    Laplace realisations, 100 steps)

Nothing here is a threshold: the file states whether "reference" stayed within the parent's spread
and by how much "predicted" differs from "reference" in the same session.
"""
import argparse
import json
import os
import sys

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
FORMS = {"reference": {}, "predicted": dict(linearize="predicted"),
         "predicted_relinearize_1": dict(linearize="predicted", relinearize=1)}
SAFETY_B, SAFETY_M, SAFETY_STEPS, LATERAL = 1024, 1000, 100, 1.0


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
    return model, nominal, to(x_ref[:P]), to(u_ref[:P]), x0, (m["Q"], m["R"], cfg)


def starts(x0, B):
    offsets = 1e-2 * np.random.default_rng(11).standard_normal((B, 4))
    offsets[0] = 0.0
    return x0 + offsets


def batch(parts, B, form, **kw):
    model, nominal, x_ref, u_ref = parts[:4]
    return closed_loop.RecedingHorizonBatch(model, nominal, x_ref, u_ref, N, RiskParams(), n_problems=B,
                                            seed=SEED, steps_per_graph=10, **FORMS[form], **kw)


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
    """The halfspace launch of one control step alone at B problems, in both forms, from the first
    step's buffers (the launch writes the record and nothing else)."""
    x0 = starts(parts[4], B)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    row = {"B": B}
    loop = batch(parts, B, "reference")
    loop.reset(x0)
    dev_form, _ = engine.prepare_sampled_halfspaces_dev(
        loop.nominal_path, loop.ego_path, H, N, RiskParams(), loop._state[0], seed=SEED,
        out=loop._record, stream=side)
    loop_p = batch(parts, B, "predicted")
    loop_p.reset(x0)
    replays = {"dev_form": graph_of(dev_form, side),
               "pred_form_shift_1": graph_of(loop_p._lin_launch(side, 1), side),
               "pred_form_shift_0": graph_of(loop_p._lin_launch(side, 0), side)}
    for _ in range(2):                       # alternated: dev, pred, pred, dev, pred, pred
        for name, replay in replays.items():
            row.setdefault(name, []).append(timed(replay))
    return row


def safety_of(parts, form):
    """100 evaluated steps of B = 1024 loops whose starts are spread laterally about the scenario's
    start: collisions, clearance and the tracking cost of the states actually visited."""
    model, nominal, x_ref, u_ref, x0, (Q, R, cfg) = parts
    along = np.asarray(cfg["ego_goal"], dtype=np.float64) - np.asarray(cfg["ego_start"], dtype=np.float64)
    across = np.array([-along[1], along[0]]) / np.linalg.norm(along)
    x0s = np.tile(x0, (SAFETY_B, 1))
    x0s[:, :2] += np.linspace(-LATERAL, LATERAL, SAFETY_B)[:, None] * across
    params = RiskParams()
    evaluate = closed_loop.LoopEvaluation(SAFETY_M, noise="laplace", robot_radius=params.robot_radius,
                                          obstacle_radius=params.obstacle_radius, seed=77)
    loop = batch(parts, SAFETY_B, form, evaluate=evaluate)
    loop.reset(x0s)
    states, inputs, info = loop.run(SAFETY_STEPS, backend="graph")
    s = loop.safety()
    dx = states[:, 1:] - x_ref[1:SAFETY_STEPS + 1]
    du = inputs - u_ref[:SAFETY_STEPS]
    Qd, Rd = (torch.from_numpy(np.ascontiguousarray(a)).to(states.device) for a in (Q, R))
    cost = torch.einsum("bti,ij,btj->b", dx, Qd, dx) + torch.einsum("bti,ij,btj->b", du, Rd, du)
    status = info[..., 0]
    clearance = s["min_clearance"]
    return {"B": SAFETY_B, "M": SAFETY_M, "steps": SAFETY_STEPS, "lateral_spread_m": LATERAL,
            "realisations_in_collision": int((clearance < 0).sum()),
            "loops_with_a_collision": int(((clearance < 0).sum(dim=1) > 0).sum()),
            "collision_rate_mean": float(s["collided"].mean()),
            "collision_rate_max": float(s["collided"].max()),
            "step_hits_total": int(s["step_hits"].sum()),
            "min_clearance_min": float(clearance.min()),
            "min_clearance_mean": float(clearance.mean()),
            "min_clearance_p05": float(torch.quantile(clearance.flatten()[::16], 0.05)),
            "tracking_cost_mean": float(cost.mean()), "tracking_cost_max": float(cost.max()),
            "solved_share": float(((status == 0) | (status == 3)).double().mean())}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_pred_times.py measures on the GPU; there is none")
    dev = torch.device("cuda", 0)
    parts = setup(dev)
    result = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "repeats": args.repeats,
              "launches": args.launches, "shape": {"O": 3, "H": H, "N": N, "P": P},
              "sampled_source_key": _native.source_key("drcvar_sampled.hip"),
              "timing": "device events around a window of back-to-back control steps (graph, 10 steps "
                        "per graph), ms per control step: median (min, max) over `repeats` windows"}
    forms = ("reference",) if args.part == "reference" else tuple(FORMS)
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
        result["halfspaces_alone"] = halfspaces_alone(dev, parts, BATCHES[-1])
        print(json.dumps(result["halfspaces_alone"]), flush=True)
        result["safety"] = {form: safety_of(parts, form) for form in FORMS}
        print(json.dumps(result["safety"]), flush=True)
        ab = {"parent": [json.load(open(f))["batch"] for f in args.ab_parent],
              "tree": [json.load(open(f))["batch"] for f in args.ab_tree]}
        result["reference_ab"] = ab
        summary = {}
        for k, B in enumerate(BATCHES):
            ref, pred = rows[k]["reference"], rows[k]["predicted"]
            ref_lo, ref_hi = min(r["ms_min"] for r in ref), max(r["ms_max"] for r in ref)
            pred_med = float(np.median([r["ms"] for r in pred]))
            ref_med = float(np.median([r["ms"] for r in ref]))
            entry = {"reference_ms_range": [ref_lo, ref_hi], "reference_ms_median": ref_med,
                     "predicted_ms_median": pred_med, "predicted_over_reference": pred_med / ref_med,
                     "predicted_within_reference_range": bool(ref_lo <= pred_med <= ref_hi)}
            if ab["parent"] and ab["tree"]:
                par = [run[k]["reference"][0] for run in ab["parent"]]
                tre = [run[k]["reference"][0] for run in ab["tree"]] + ref
                lo, hi = min(r["ms_min"] for r in par), max(r["ms_max"] for r in par)
                t_lo, t_hi = min(r["ms_min"] for r in tre), max(r["ms_max"] for r in tre)
                entry["parent_reference_ms_range"] = [lo, hi]
                entry["tree_reference_ms_range"] = [t_lo, t_hi]
                entry["reference_ranges_overlap"] = bool(t_lo <= hi and lo <= t_hi)
            summary[str(B)] = entry
        result["summary"] = summary
        print(json.dumps(summary), flush=True)
    out = args.out or os.path.join(REPO, "profiles", "closed_loop", "closed_loop_pred_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
