#!/usr/bin/env python3
"""The HEAD simulator's training script (src/salp/environments/train_robot.py: SAC "MlpPolicy", lr 3e-4, buffer 1e5,
batch 512, ent_coef "auto", gamma 0.99, tau 0.005, 8 SubprocVecEnv workers) on the batched HIP simulator:
    python examples/train_robot_sac.py --envs 4096 --steps 300
    python examples/train_robot_sac.py --envs 4096 --steps 320 --in-kernel 16 --hidden 64,64
One env step is one whole breathing cycle of every robot (contract, jet, coast).
--in-kernel H collects H breathing cycles per robot in ONE launch: the actor runs inside the rollout kernel as a
`policy.GaussianPolicy` (`sac.collect_in_kernel`: sampled actions, terminal rows kept), which needs hidden layers of at most
64 units (--hidden); the agent then makes `updates_per_step` updates per collected cycle."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from underwater_swimmer_rl_amd.robot_env import SalpRobotVectorEnv
from underwater_swimmer_rl_amd.sac import SAC, SACConfig, DeviceReplayBuffer, collect_in_kernel, train_sac, train_sac_graphed


def train_in_kernel(env, agent, total_vector_steps, horizon):
    """Collect `horizon` cycles per launch with the actor inside the rollout kernel, then learn; the metrics of train_sac
    that this loop has."""
    import torch
    cfg = agent.cfg
    buffer = DeviceReplayBuffer(cfg.buffer_size, env.obs_dim, env.act_dim, agent.device)
    env.reset()
    handle, steps, last = None, 0, {}
    t0 = time.perf_counter()
    while steps < total_vector_steps:
        handle = collect_in_kernel(env, agent, buffer, horizon, handle)
        steps += horizon
        if steps >= cfg.learning_starts and buffer.size >= cfg.batch_size:
            for _ in range(horizon * cfg.updates_per_step):
                last = agent.update(buffer.sample(cfg.batch_size))
    torch.cuda.synchronize()
    return {"wall_s": time.perf_counter() - t0, "vector_steps": steps, "env_steps": steps * env.num_envs,
            "updates": agent.updates, "noise_step": handle.noise_step, **{k: float(v) for k, v in last.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300, help="vector env steps (breathing cycles per robot)")
    ap.add_argument("--learning-starts", type=int, default=10)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--in-kernel", type=int, default=0, metavar="H",
                    help="collect H cycles per launch with the actor sampled inside the rollout kernel (needs --hidden <= 64)")
    ap.add_argument("--hidden", default=None, help="actor / critic hidden sizes, e.g. 64,64 (default: the preset's)")
    args = ap.parse_args()
    env = SalpRobotVectorEnv(args.envs, device="cuda:0", seed=0)
    cfg = SACConfig.from_preset("salp_robot")
    cfg.learning_starts = args.learning_starts
    if args.hidden:
        cfg.hidden_sizes = tuple(int(h) for h in args.hidden.split(","))
    agent = SAC(env.obs_dim, env.act_dim, cfg, device="cuda:0", seed=0,
                act_low=env.single_action_space.low, act_high=env.single_action_space.high)
    if args.in_kernel > 0:
        m = train_in_kernel(env, agent, args.steps, args.in_kernel)
    else:
        run = train_sac if args.eager else train_sac_graphed
        m = run(env, agent, args.steps)
        m["first_target_reached_wall_s"] = m.pop("first_food_wall_s")
        m["first_target_reached_vector_step"] = m.pop("first_food_vector_step")
    m["config"] = {"envs": args.envs, "batch_size": cfg.batch_size, "buffer_size": cfg.buffer_size}
    print(json.dumps(m))
    env.close()


if __name__ == "__main__":
    main()
