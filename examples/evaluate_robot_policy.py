#!/usr/bin/env python3
"""Cross-entropy search over LINEAR policies of the jet-propelled robot (the HEAD simulator, `SalpRobotVectorEnv`), the
whole population inside the rollout kernel: 64 policies x 64 robots per launch (`rollout_policy` with a stacked
`MLPPolicy`), ONE launch per generation of `--cycles` breathing cycles each, the weights refreshed in place between
generations (`handle.update`, no re-allocation).  A policy is a = clip(W obs + b, -1, 1) * scale + shift on the env's Box
(contraction, coast time, nozzle yaw), 21 parameters; its score is the mean over its robots of the summed reward (progress
towards the target, heading, the bonus for reaching it).  No pass threshold: it prints the scores per generation and the
score of a policy that always jets straight ahead, on the same episodes.  Needs the GPU.
`--whole-episodes` scores a policy the way the reference's test_robot.py does — one episode per robot, run to its end, at
most 500 cycles — with `evaluate_policy(handle, 500, first_episode=True)`: no per-step output, one summary record per
robot, and a robot whose episode has ended is not simulated any further.  It prints the mean first-episode return, the
fraction of robots that reached their target and the Euler steps spent.
    python examples/evaluate_robot_policy.py [--policies P] [--robots-per-policy E] [--generations G] [--cycles T]
                                             [--whole-episodes]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from underwater_swimmer_rl_amd.policy import MLPPolicy  # noqa: E402
from underwater_swimmer_rl_amd.robot_env import SalpRobotVectorEnv  # noqa: E402

SCALE, SHIFT = np.array([0.5, 0.05, 1.0], np.float32), np.array([0.5, 0.05, 0.0], np.float32)   # the Box with coast <= 1 s


def population(theta):
    """theta float32 [P, 3, 7] -> P linear policies (W = theta[..., :6], b = theta[..., 6])."""
    P = theta.shape[0]
    return MLPPolicy([(theta[..., :6], theta[..., 6])], np.tile(SCALE, (P, 1)), np.tile(SHIFT, (P, 1)), "clip")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policies", type=int, default=64)
    ap.add_argument("--robots-per-policy", type=int, default=64)
    ap.add_argument("--generations", type=int, default=6)
    ap.add_argument("--cycles", type=int, default=24)
    ap.add_argument("--elite", type=float, default=0.125)
    ap.add_argument("--whole-episodes", action="store_true", help="score by each robot's first whole episode (at most 500 cycles)")
    args = ap.parse_args()
    P, E, T = args.policies, args.robots_per_policy, args.cycles
    env = SalpRobotVectorEnv(num_envs=P * E, seed=0)
    rng = np.random.default_rng(0)
    center, spread = np.zeros((3, 7)), np.full((3, 7), 1.0)
    theta = (center + spread * rng.standard_normal((P, 3, 7))).astype(np.float32)
    handle = env.make_policy(population(theta))

    def scores():
        env.reset()
        out = env.rollout_policy(handle, T, want_actions=False)
        return out["reward"].sum(0).view(P, E).mean(1), int(out["inner_steps"].sum())

    def episode_scores():
        env.reset()
        v = env.evaluate_policy(handle, 500, first_episode=True)
        print(f"    whole episodes: mean first-episode return {float(v['first_return'].mean()):8.2f}, reached "
              f"{float((v['first_end'] == 1).double().mean()):.3f}, {int(v['euler_steps'].sum())} Euler steps", flush=True)
        return v["first_return"].view(P, E).mean(1).float(), int(v["euler_steps"].sum())

    if args.whole_episodes:
        scores, T = episode_scores, 500
    n_elite = max(2, int(args.elite * P))
    t0, euler = time.perf_counter(), 0
    for g in range(args.generations):
        if g:
            theta = (center + spread * rng.standard_normal((P, 3, 7))).astype(np.float32)
            handle.update(torch.as_tensor(population(theta).pack(), device=env.device))
        s, steps = scores()
        euler += steps
        elite = torch.topk(s, n_elite).indices.cpu().numpy()
        center, spread = theta[elite].mean(0), np.maximum(theta[elite].std(0), 1e-3)
        print(f"generation {g}: best {float(s.max()):8.2f}  elite mean {float(s[elite].mean()):8.2f}  population mean {float(s.mean()):8.2f}", flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    straight = np.zeros((P, 3, 7), np.float32)
    straight[:, 0, 6] = 1.0                       # full contraction, shortest coast, nozzle straight
    straight[:, 1, 6] = -1.0
    handle.update(population(straight).pack())
    print(f"always straight ahead: {float(scores()[0].mean()):8.2f}")
    print(f"{args.generations} generations x {P} policies x {E} robots x {T} cycles in {dt:.2f} s "
          f"({euler / dt:.3g} Euler steps/s, one launch per generation)")
    env.close()


if __name__ == "__main__":
    main()
