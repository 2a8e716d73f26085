"""Golden vectors of the Monte Carlo collision evaluation, produced by the REFERENCE's own code
(run in the build container only; only the ``.npz`` data travels).

    python tests/golden/make_golden_mc.py --reference <path to the reference checkout>

Writes ``tests/golden/monte_carlo/clearance_ref.npz`` (a subdirectory: ``conftest.golden_files()``
globs ``tests/golden/*.npz`` for the halfspace parity tests).  ``simulation.obstacles`` and
``evaluation.metrics`` import as they are; ``simulation.environment`` and ``simulation.planner``
import ``cvxpy`` at module level, which is stubbed as in ``make_golden_ref.py`` (nothing here calls
into it).

Recipe: the ``multi_obstacle`` scenario's nominal paths (``generate_nominal_trajectory``) truncated
to 21 steps; two ego trajectories, the planner's straight line (horizon 20) and a copy shifted
sideways by ``SHIFT`` so that its collision rate under the Laplace noise is neither 0 nor 1; then
``np.random.seed(42)`` and 16 realisations, each ``generate_laplace_realization`` per obstacle in
order followed by ``compute_distance_to_collision`` per ego (main.py:128-138), and
``safety_metrics`` of the per-realisation minima.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS, REALIZATIONS, SEED = 21, 16, 42
SHIFT = (0.0, 0.55)
NOISE_COV = np.diag([0.01, 0.01])            # simulation/obstacles.py:134


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    sys.modules.setdefault("cvxpy", mock.MagicMock(name="cvxpy-stub"))
    sys.path.insert(0, args.reference)
    from config import parameters as P
    from config.scenarios import get_scenario_config
    from core.dynamics import create_double_integrator_matrices
    from evaluation.metrics import safety_metrics
    from simulation.environment import SafetyFilteringEnvironment
    from simulation.obstacles import generate_laplace_realization, generate_nominal_trajectory
    from simulation.planner import ReferenceTrajectoryPlanner

    cfg = get_scenario_config("multi_obstacle")
    env = SafetyFilteringEnvironment(ROBOT_RADIUS=P.ROBOT_RADIUS, OBSTACLE_RADIUS=P.OBSTACLE_RADIUS,
                                     HORIZON=STEPS - 1, DT=P.DT, ALPHA=P.ALPHA, DELTA=P.DELTA,
                                     EPSILON=P.EPSILON)
    A, B, C = create_double_integrator_matrices(P.DT)
    n_steps = int(P.SIM_TIME / P.DT)
    nominal = np.stack([generate_nominal_trajectory(ob["start"], ob["direction"], ob.get("speed", 1.0),
                                                    n_steps, P.DT)[:STEPS] for ob in cfg["obstacles"]])
    planner = ReferenceTrajectoryPlanner(A, B, C, P.Q_WEIGHT * np.eye(4), P.R_WEIGHT * np.eye(2),
                                         STEPS - 1, P.DT)
    x_ref, _, _ = planner.straight_line_trajectory(cfg["ego_start"], cfg["ego_goal"])
    shifted = x_ref.copy()
    shifted[:, :2] += np.asarray(SHIFT)
    egos = np.stack([x_ref, shifted])                                  # [2, 21, 4] states
    np.random.seed(SEED)
    realizations = np.empty((REALIZATIONS,) + nominal.shape)
    distances = np.empty((len(egos), REALIZATIONS, STEPS))
    for m in range(REALIZATIONS):
        real = [generate_laplace_realization(nom, NOISE_COV, P.DT) for nom in nominal]
        realizations[m] = np.stack(real)
        for k, ego in enumerate(egos):
            distances[k, m] = env.compute_distance_to_collision(ego, real)
    keys = sorted(safety_metrics(distances[0].min(axis=1)))
    table = np.array([[float(safety_metrics(distances[k].min(axis=1))[key]) for key in keys]
                      for k in range(len(egos))])
    os.makedirs(os.path.join(HERE, "monte_carlo"), exist_ok=True)
    path = os.path.join(HERE, "monte_carlo", "clearance_ref.npz")
    meta = dict(source="reference simulation.obstacles / simulation.environment / evaluation.metrics "
                       "(cvxpy stubbed)", scenario="multi_obstacle", seed=SEED, shift=list(SHIFT),
                robot_radius=P.ROBOT_RADIUS, obstacle_radius=P.OBSTACLE_RADIUS, dt=P.DT)
    np.savez(path, nominal=nominal, egos=egos, realizations=realizations, distances=distances,
             metric_keys=np.array(keys), metrics=table, noise_cov=NOISE_COV,
             radii=np.array([P.ROBOT_RADIUS, P.OBSTACLE_RADIUS]), meta=np.asarray(json.dumps(meta)))
    print(f"wrote {path}: nominal {nominal.shape} egos {egos.shape} distances {distances.shape}; "
          f"min clearance of the nominal paths {[float(distances[k].min()) for k in range(len(egos))]}")


if __name__ == "__main__":
    main()
