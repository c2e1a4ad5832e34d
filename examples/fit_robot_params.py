#!/usr/bin/env python3
"""Fits the HEAD robot model to a "measured" run by batched trajectory comparison (robot_compare, one GPU call per
round of 65536 candidates).  The measured run is synthetic: a hidden parameter set plus noise.  A few rounds of the
cross-entropy method over the drag coefficients, the nozzle area and the dry mass; the other parameters stay at their
defaults.  No pass threshold: it prints the fitted values next to the hidden ones.
    python examples/fit_robot_params.py [--candidates N] [--rounds R] [--cycles T]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from underwater_swimmer_rl_amd.robot_compare import ROBOT_PARAM_NAMES, compare_actions_with_states, robot_params  # noqa: E402

FIT = ("drag_coefficient_min", "drag_coefficient_max", "nozzle_area", "dry_mass")
HIDDEN = dict(drag_coefficient_min=0.33, drag_coefficient_max=1.18, nozzle_area=0.000135, dry_mass=1.22)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--cycles", type=int, default=24)
    ap.add_argument("--elite", type=float, default=0.02)
    args = ap.parse_args()
    dev = "cuda:0"
    rng = np.random.default_rng(1)
    T, N = args.cycles, args.candidates
    # a varied breathing-cycle sequence in the reference's units: contraction m, coast s, nozzle yaw rad
    a = np.stack([rng.uniform(0.3, 1.0, T), rng.uniform(0.0, 0.15, T), rng.uniform(-1, 1, T)], 1).astype(np.float32)
    actions = a.astype(np.float64) * np.array([0.06, 10.0, np.pi / 2])

    truth = compare_actions_with_states(actions, None, dict(HIDDEN))["actual_states"][0]
    noise = torch.as_tensor(rng.normal(0, 1, (T, 6)) * np.array([0.005, 0.005, 0.002, 0.002, 0.01, 0.005]), device=dev)
    measured = truth + noise

    # search box (x0.5 .. x1.5 around the defaults), CEM in log space
    d = robot_params(1, dev)[:, 0].cpu().numpy()
    rows = {name: i for i, name in enumerate(ROBOT_PARAM_NAMES)}
    center = np.zeros(len(FIT))
    spread = np.full(len(FIT), np.log(1.5) / 2)
    g = torch.Generator(device=dev).manual_seed(0)
    n_elite = max(8, int(args.elite * N))
    t0 = time.perf_counter()
    for r in range(args.rounds):
        z = torch.randn((len(FIT), N), generator=g, device=dev, dtype=torch.float64)
        logs = torch.as_tensor(center, device=dev)[:, None] + torch.as_tensor(spread, device=dev)[:, None] * z
        logs = logs.clamp(np.log(0.5), np.log(1.5))
        P = robot_params(N, dev)
        for j, name in enumerate(FIT):
            P[rows[name]] = float(d[rows[name]]) * torch.exp(logs[j])
        P[rows["drag_coefficient_max"]] = torch.maximum(P[rows["drag_coefficient_max"]], P[rows["drag_coefficient_min"]] + 1e-3)
        out = compare_actions_with_states(actions, measured, P, metrics_only=True)
        score = out["position_error"] + 0.2 * out["velocity_error"] + 0.1 * out["angle_error"]
        elite = torch.topk(score, n_elite, largest=False).indices
        center = logs[:, elite].mean(1).cpu().numpy()
        spread = np.maximum(logs[:, elite].std(1).cpu().numpy(), 1e-4)
        best = int(elite[0])
        print(f"round {r}: best score {score[best].item():.5f} m  mean position error {out['position_error'][best].item():.5f} m  "
              + "  ".join(f"{name}={P[rows[name], best].item():.6g}" for name in FIT), flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{args.rounds} rounds x {N} candidates x {T} cycles in {dt:.2f} s (wall, including host work)")
    fitted = {name: float(d[rows[name]] * np.exp(center[j])) for j, name in enumerate(FIT)}
    print(f"{'parameter':<22}{'hidden':>12}{'fitted':>12}{'default':>12}")
    for name in FIT:
        print(f"{name:<22}{HIDDEN[name]:>12.6g}{fitted[name]:>12.6g}{d[rows[name]]:>12.6g}")


if __name__ == "__main__":
    main()
