"""Times the out-of-sample collision evaluation inside the receding-horizon loops
(simulation/closed_loop.py, evaluate=LoopEvaluation(...); drcvar_loop_clearance_f64) and writes
profiles/closed_loop/closed_loop_eval_times.json.

    python scripts/micro/closed_loop_eval_times.py --part plain [--tree DIR] --out FILE
    python scripts/micro/closed_loop_eval_times.py [--out FILE] --ab-parent FILE ... --ab-tree FILE ...

Protocol of closed_loop_batch_times.py: device-event time over a window of `--steps` back-to-back
control steps after a warm-up window, the median and the spread (min, max) of `--repeats` windows,
in ms per control step; main.py's shape (3 obstacles, H = 30, N = 20, P = 151).

  --part plain   only RecedingHorizonBatch with evaluate=None at B = 1 and 1024 (`graph`, 10 steps
                 per graph), importing the package from --tree: run on a build of the parent commit
                 and on this tree, alternated in one session, and hand the files to the full run
  (full run)     1. the plain rows again, and whether the parent's and this tree's window ranges
                    overlap;
                 2. the step with an evaluation of M = 1000 and 10000 Laplace realisations at
                    B = 1, 64, 1024, and the evaluation launch alone (a graph of one launch), also
                    across realisations-per-thread settings;
                 3. the launch at B = 1024, M = 10000, O = 3 (3.07e7 points) for both noise kinds
                    against min_clearance_device at its (3, 30, 1e6) shape, time per point;
                 4. the same statistics after the fact: B host-driven min_clearance_device calls
                    on the logged states of a 100-step run (B = 1024, M = 1000), end to end.
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
ap.add_argument("--part", choices=("all", "plain"), default="all")
ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
ap.add_argument("--ab-parent", nargs="*", default=[])
ap.add_argument("--ab-tree", nargs="*", default=[])
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
REPO = os.path.abspath(args.tree)
sys.path.insert(0, REPO)

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.config.scenarios import (  # noqa: E402
    get_scenario_config)
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core.mpc_filter import MPCModel  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.evaluation import monte_carlo as mc  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import closed_loop  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import obstacles as ob  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.planner import (  # noqa: E402
    ReferenceTrajectoryPlanner)

SEED, H, N, P, DT = 5, 30, 20, 151, 0.2
RADII = dict(robot_radius=0.3, obstacle_radius=0.3)


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
    return model, nominal, to(x_ref[:P]), to(u_ref[:P]), x0


def starts(x0, B):
    offsets = 1e-2 * np.random.default_rng(11).standard_normal((B, 4))
    offsets[0] = 0.0
    return x0 + offsets


def batch(parts, B, **kw):
    model, nominal, x_ref, u_ref, _ = parts
    return closed_loop.RecedingHorizonBatch(model, nominal, x_ref, u_ref, N, RiskParams(),
                                            n_problems=B, seed=SEED, steps_per_graph=10, **kw)


def loop_windows(loop, x0):
    """ms per control step of `--repeats` windows of `--steps` steps on `graph`, each from a reset."""
    loop.reset(x0)
    loop.run(args.steps, backend="graph")                    # captures / warms up
    ms = []
    for _ in range(args.repeats):
        loop.reset(x0)                                       # same first step: the capture is kept
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loop.run(args.steps, backend="graph")
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / args.steps)
    return spread(ms)


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


def plain_rows(parts):
    return {str(B): loop_windows(batch(parts, B), starts(parts[4], B)) for B in (1, 1024)}


def launch_alone(dev, parts, B, M, noise="laplace", per_thread=0):
    """The evaluation launch alone at B problems in their start states, from a graph of one launch."""
    model, nominal, _, _, x0 = parts
    O = nominal.shape[0]
    f64 = dict(dtype=torch.float64, device=dev)
    x0_d = torch.from_numpy(starts(x0, B)).to(dev)
    state = torch.tensor([[0, 7]], dtype=torch.int64, device=dev).repeat(B, 1)
    min_d2 = torch.full((B, M), float("inf"), **f64)
    hits = torch.zeros((B, 65), dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    launch = mc.prepare_loop_clearance_step(
        x0_d, np.asarray(model.C, dtype=np.float64), nominal.repeat(B, 1, 1), O, state, min_d2, hits,
        step_begin=0, log_rows=64, noise=noise, seed=3, realizations_per_thread=per_thread,
        stream=side, **RADII)
    with torch.cuda.stream(side):
        launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch()
    row = timed(graph.replay)
    row["points"] = B * M * O
    row["G_points_per_s"] = row["points"] / (row["ms"] * 1e-3) / 1e9
    return row


def existing_kernel(dev, noise, K):
    """min_clearance_device at its (3, 30, 1e6) shape: ms per call and points per second."""
    O, T, M = 3, 30, 1_000_000
    rng = np.random.default_rng(2)
    ego = torch.from_numpy(rng.uniform(-2, 2, size=(K, T, 2))).to(dev)
    nom = torch.from_numpy(rng.uniform(-2, 2, size=(O, T, 2))).to(dev)
    out = torch.empty((K, M), dtype=torch.float64, device=dev)
    row = timed(lambda: mc.min_clearance_device(ego, nom, M, noise=noise, seed=3, out=out, **RADII))
    row["points"] = O * T * M
    row["G_points_per_s"] = row["points"] / (row["ms"] * 1e-3) / 1e9
    return row


def after_the_fact(dev, parts, B, M):
    """A 100-step run without an evaluation, then B host-driven min_clearance_device calls on the
    logged positions (with the per-step counts): host clock around the calls and a synchronise."""
    model, nominal, _, _, x0 = parts
    loop = batch(parts, B)
    loop.reset(starts(x0, B))
    states, _, _ = loop.run(args.steps, backend="graph")
    C = torch.as_tensor(np.asarray(model.C, dtype=np.float64)).to(dev)
    ego = (states @ C.T).contiguous()                                     # [B, steps + 1, 2]
    nom = nominal[:, :args.steps + 1].contiguous()
    out = torch.empty((1, M), dtype=torch.float64, device=dev)
    ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in range(B):
            mc.min_clearance_device(ego[b:b + 1], nom, M, seed=3, stream_offset=b, step_hits=True,
                                    out=out, **RADII)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"B": B, "M": M, "steps": args.steps, "calls": B, **spread(ms)}


def main():
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_eval_times.py measures on the GPU; there is none")
    dev = torch.device("cuda", 0)
    parts = setup(dev)
    result = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "repeats": args.repeats,
              "launches": args.launches, "shape": {"O": 3, "H": H, "N": N, "P": P},
              "clearance_source_key": _native.source_key("drcvar_clearance.hip"),
              "timing": "device events around a window of back-to-back control steps (or graph "
                        "replays of one launch), ms per step (per replay): median (min, max) over "
                        "`repeats` windows"}
    result["plain"] = plain_rows(parts)
    print(json.dumps(result["plain"]), flush=True)
    if args.part == "all":
        Ev = closed_loop.LoopEvaluation
        cost = []
        for M in (1000, 10000):
            for B in (1, 64, 1024):
                row = {"B": B, "M": M}
                row["step_with_evaluation"] = loop_windows(
                    batch(parts, B, evaluate=Ev(M, seed=3, **RADII)), starts(parts[4], B))
                row["step_plain"] = loop_windows(batch(parts, B), starts(parts[4], B))
                row["launch_alone"] = launch_alone(dev, parts, B, M)
                row["added_ms"] = row["step_with_evaluation"]["ms"] - row["step_plain"]["ms"]
                cost.append(row)
                print(json.dumps(row), flush=True)
        result["cost"] = cost
        result["per_thread_sweep"] = [
            {"B": B, "M": M, "per_thread": per, **launch_alone(dev, parts, B, M, per_thread=per)}
            for B, M in ((1024, 10000), (1024, 1000), (64, 10000), (1, 10000))
            for per in (0, 1, 2, 4, 8, 16, 32)]
        print(json.dumps(result["per_thread_sweep"]), flush=True)
        versus = {}
        for noise in ("laplace", "gaussian"):
            new = launch_alone(dev, parts, 1024, 10000, noise)
            old = {f"K{K}": existing_kernel(dev, noise, K) for K in (1, 4)}
            versus[noise] = {"loop_launch": new, "existing": old, "time_per_point_ratio_vs_K1":
                             old["K1"]["G_points_per_s"] / new["G_points_per_s"],
                             "time_per_point_ratio_vs_K4":
                             old["K4"]["G_points_per_s"] / new["G_points_per_s"]}
        result["versus_existing_kernel"] = versus
        print(json.dumps(versus), flush=True)
        result["after_the_fact"] = after_the_fact(dev, parts, 1024, 1000)
        in_graph = next(r for r in cost if r["B"] == 1024 and r["M"] == 1000)
        result["after_the_fact"]["in_graph_added_ms_for_the_run"] = in_graph["added_ms"] * args.steps
        print(json.dumps(result["after_the_fact"]), flush=True)
        ab = {"parent": [json.load(open(f))["plain"] for f in args.ab_parent],
              "tree": [json.load(open(f))["plain"] for f in args.ab_tree]}
        result["plain_ab"] = ab
        if ab["parent"] and ab["tree"]:
            overlap = {}
            for B in ("1", "1024"):
                p = (min(r[B]["ms_min"] for r in ab["parent"]), max(r[B]["ms_max"] for r in ab["parent"]))
                t = (min(r[B]["ms_min"] for r in ab["tree"]), max(r[B]["ms_max"] for r in ab["tree"]))
                overlap[B] = {"parent_ms_range": p, "tree_ms_range": t,
                              "overlap": bool(p[0] <= t[1] and t[0] <= p[1])}
            result["plain_ranges_overlap"] = overlap
    out = args.out or os.path.join(REPO, "profiles", "closed_loop", "closed_loop_eval_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
