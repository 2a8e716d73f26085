"""Times the receding-horizon loop (simulation/closed_loop.py) and the device-state form of the
sampled-halfspace launch, and writes profiles/closed_loop/closed_loop_times.json.

    python scripts/micro/closed_loop_times.py [--out FILE] [--ab FILE ...]
    python scripts/micro/closed_loop_times.py --part base [--tree DIR] --out FILE

Every figure is device-event time over back-to-back steps after a warm-up: the median and the
spread (min, max) of `--repeats` windows, in ms per launch or per control step.

  launch      drcvar_sampled_halfspaces_f64 (base) against drcvar_sampled_halfspaces_f64_dev, each
              replayed from a graph of one launch, at C3 (10 x 20 x 1000) and C4 (64 x 30 x 5000);
              the device state is not advanced, so both do the same work
  loop        ms per control step of the `graph` (1 and 10 steps per graph), `launches` and
              `reference` backends over 100 steps, beside the device-state halfspace launch and the solver launch timed alone
              (graphs of one launch), at main.py's shape (3 obstacles, H = 30, N = 20, P = 151)
              and a C3-like shape (10 obstacles, H = 20, N = 1000)
  --part base only the base entry's graph replay, importing the package from --tree: run once on
              this tree and once on a build of the parent commit, alternated in one session, and
              hand the files to the full run with --ab (the base entry must not move)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--part", choices=("all", "base"), default="all")
ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
ap.add_argument("--ab", nargs="*", default=[])
ap.add_argument("--launches", type=int, default=10)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
REPO = os.path.abspath(args.tree)
sys.path.insert(0, REPO)

from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd import _native, engine, synthetic  # noqa: E402
from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.engine import RiskParams  # noqa: E402

SEED = 5
LAUNCH_SHAPES = [("C3", 10, 20, 1000), ("C4", 64, 30, 5000)]


def spread(ms):
    return {"ms": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def timed(fn, count, repeats, warmup=3, before=None):
    """ms per call of fn: windows of `count` back-to-back calls between two device events."""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        if before is not None:
            before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(count):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / count)
    return spread(ms)


def graph_of(make, dev):
    """A graph of the one launch `make(stream)` prepares (run once eagerly first)."""
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        launch = make(side)
        launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch()
    return graph.replay


def launch_inputs(O, T, dev):
    rng = np.random.default_rng(O * 1000 + T)
    nominal = torch.from_numpy(rng.uniform(-5.0, 5.0, size=(O, T, 2))).to(dev)
    ego = synthetic.straight_line_ego(T, dev, start=(-7.0, -6.0), goal=(-5.5, -5.5))
    return nominal, ego


def base_rows(dev):
    rows = []
    for name, O, T, N in LAUNCH_SHAPES:
        nominal, ego = launch_inputs(O, T, dev)
        out = torch.empty((O, T, 8), dtype=torch.float64, device=dev)
        base = graph_of(lambda s: engine.prepare_sampled_halfspaces(
            nominal, ego, N, RiskParams(), seed=SEED, stream_offset=3, out=out, stream=s)[0], dev)
        rows.append({"shape": name, "O": O, "T": T, "N": N,
                     "base_graph": timed(base, args.launches, args.repeats)})
    return rows


def launch_rows(dev):
    rows = []
    for name, O, T, N in LAUNCH_SHAPES:
        nominal, ego = launch_inputs(O, T, dev)
        out = torch.empty((O, T, 8), dtype=torch.float64, device=dev)
        out_dev = torch.empty((O, T, 8), dtype=torch.float64, device=dev)
        state = torch.tensor([3, 0], dtype=torch.int64, device=dev)
        base = graph_of(lambda s: engine.prepare_sampled_halfspaces(
            nominal, ego, N, RiskParams(), seed=SEED, stream_offset=3, out=out, stream=s)[0], dev)
        devf = graph_of(lambda s: engine.prepare_sampled_halfspaces_dev(
            nominal, ego, T, N, RiskParams(), state, seed=SEED, out=out_dev, stream=s)[0], dev)
        row = {"shape": name, "O": O, "T": T, "N": N}
        # alternated, so that a drift of the device shows in both
        row["base_graph"] = timed(base, args.launches, args.repeats)
        row["dev_graph"] = timed(devf, args.launches, args.repeats)
        row["base_graph_again"] = timed(base, args.launches, args.repeats)
        row["dev_graph_again"] = timed(devf, args.launches, args.repeats)
        torch.cuda.synchronize()
        row["records_equal"] = bool(torch.equal(out, out_dev))
        lo = min(row["base_graph"]["ms_min"], row["base_graph_again"]["ms_min"])
        hi = max(row["base_graph"]["ms_max"], row["base_graph_again"]["ms_max"])
        row["dev_within_base_spread"] = bool(lo <= row["dev_graph"]["ms"] <= hi)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def loop_rows(dev):
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.core.mpc_filter import (
        MPCModel, filter_batch, record_views)
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation import obstacles as ob
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.closed_loop import (
        RecedingHorizonFilter)
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.simulation.planner import (
        ReferenceTrajectoryPlanner)
    from dr_cvar_mpc_safety_filter_motion_planning_collison_avoidance_amd.config.scenarios import (
        get_scenario_config)
    m = np.load(os.path.join(REPO, "tests", "golden", "mpc_multi_obstacle_h30.npz"), allow_pickle=False)
    cfg = get_scenario_config("multi_obstacle")
    P, dt = 151, 0.2
    planner = ReferenceTrajectoryPlanner(m["A"], m["B"], m["C"], m["Q"], m["R"], P, dt)
    x_ref, u_ref, _ = planner.straight_line_trajectory(cfg["ego_start"], cfg["ego_goal"])
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x_ref, u_ref = to(x_ref[:P]), to(u_ref[:P])
    x0 = np.zeros(4)
    x0[:2] = cfg["ego_start"]
    specs = [(o["start"], o["direction"], o["speed"]) for o in cfg["obstacles"]]
    rng = np.random.default_rng(10)
    more = [(rng.uniform(-4, 4, 2), rng.uniform(-1, 1, 2), 0.7) for _ in range(7)]
    rows = []
    for name, obst, H, N in (("main.py (3 x 30 x 20)", specs, 30, 20),
                             ("C3-like (10 x 20 x 1000)", specs + more, 20, 1000)):
        nominal = to(np.stack([ob.generate_nominal_trajectory(s, d, v, P, dt)[:P] for s, d, v in obst]))
        model = MPCModel(m["A"], m["B"], m["C"], m["Q"], m["R"], H, tuple(m["u_bounds"]),
                         tuple(m["p_bounds"]), device=dev)
        row = {"shape": name, "O": len(obst), "H": H, "N": N, "P": P, "steps": args.steps}
        status = {}
        for label, backend, per_graph in (("graph", "graph", 1), ("graph_10_steps", "graph", 10),
                                          ("launches", "launches", 1), ("reference", "reference", 1)):
            loop = RecedingHorizonFilter(model, nominal, x_ref, u_ref, N, RiskParams(), seed=SEED,
                                         steps_per_graph=per_graph)
            result = []

            def window():
                result[:] = loop.run(args.steps, backend=backend)

            loop.reset(x0)
            window()                                   # captures / warms up
            ms = []
            for _ in range(args.repeats):
                loop.reset(x0)                         # same first step: the capture is kept
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                window()
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b) / args.steps)
            row[label] = spread(ms)
            status[label] = result[2][:, 0].cpu().numpy()
            row[label + "_solved_steps"] = int(np.isin(status[label], (0, 3)).sum())
            row[label + "_mean_iterations"] = float(result[2][:, 1].mean())
        row["same_statuses"] = all(np.array_equal(s, status["reference"]) for s in status.values())
        # the two launches of a step alone, each replayed from a graph of one launch
        loop = RecedingHorizonFilter(model, nominal, x_ref, u_ref, N, RiskParams(), seed=SEED)
        loop.reset(x0)
        hs = graph_of(lambda s: engine.prepare_sampled_halfspaces_dev(
            nominal, loop.ego_path, H, N, RiskParams(), loop._state, seed=SEED, out=loop._record,
            stream=s)[0], dev)
        hs_h, hs_g = record_views(loop._record, "dr_cvar")
        solver = graph_of(lambda s: (lambda: filter_batch(
            model, hs_h, hs_g, loop._x0, loop._x_ref_win, loop._u_fb, workspace=loop._workspace,
            stream=s, out=(loop._x, loop._u, loop._info))), dev)
        row["halfspaces_alone"] = timed(hs, args.launches, args.repeats)
        row["solver_alone"] = timed(solver, args.launches, args.repeats)
        row["halfspaces_plus_solver_ms"] = row["halfspaces_alone"]["ms"] + row["solver_alone"]["ms"]
        row["graph_not_slower_than_reference"] = bool(row["graph"]["ms"] <= row["reference"]["ms_max"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    if not torch.cuda.is_available():
        raise SystemExit("closed_loop_times.py measures on the GPU; there is none")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "launches": args.launches, "steps": args.steps,
              "repeats": args.repeats, "kernel_source_key": _native.source_key("drcvar_sampled.hip"),
              "halfspace_source_key": _native.source_key(),
              "timing": "device events around back-to-back graph replays / control steps, ms each: "
                        "median (min, max) over `repeats` windows"}
    if args.part == "base":
        result["base_entry"] = base_rows(dev)
    else:
        result["launch"] = launch_rows(dev)
        result["loop"] = loop_rows(dev)
        result["base_entry_ab"] = [json.load(open(f)) | {"file": os.path.basename(f)} for f in args.ab]
    out = args.out or os.path.join(REPO, "profiles", "closed_loop", "closed_loop_times.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
