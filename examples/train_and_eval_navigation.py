#!/usr/bin/env python3
"""Train SAC on the batched simulator, then score the policy with the reference's navigation protocol
(eval/collect_navigation_data.py restated in underwater_swimmer_rl_amd.navigation_eval): 100 trials from
(150, 300) to a goal at (650, 300) with a random initial heading; the reference's published policy scores
success 1.00, 1774 +/- 254 steps, path ratio 1.17 (eval/results/navigation_stats_20251207_165158.json).
    python examples/train_and_eval_navigation.py --envs 4096 --iters 30000
Training env: single_food_long_horizon.yaml parameters; learner: that file's agent block, scaled to the batch
(a larger minibatch and several updates per vector step: 4096 new transitions arrive per step).
Measured on one MI355X with
    --iters 60000 --segments 6 --updates-per-step 4 --batch 4096 --auto-alpha --reward-scale 0.1 --lr 1e-4
(350 s for 2.5e8 env-steps, 2.4e5 updates and 7 evaluations): after the first 58 s the deterministic policy reaches the
goal in 99 of 100 trials (1766 +/- 220 steps, path ratio 1.175, straightness 0.864), after 117 s in 100 of 100 (1713 +/-
138, 1.137, 0.883); the kept checkpoint scores 100 of 100 on fresh headings with 1702 +/- 135 steps, 1.127, 0.892.
The scripted pursuit baseline: 99 of 100, 1817 +/- 216, 1.175, 0.860.  The reference's published policy: 100 of 100,
1774 +/- 254, 1.173, 0.863.  (The YAML's learner as is - fixed alpha 0.2, batch 256, unscaled reward - oscillates at
this update-to-data ratio; that is the only reason for the flags above.)
Those figures were taken with `run_navigation_trials` (one kernel launch per env-step).  The evaluations now run the whole
trial loop in one launch (`run_navigation_trials_in_kernel`, salp_vec_evaluate_navigation) whenever the actor fits
`MLPPolicy.from_actor` (up to two hidden layers of 16-64 units), and fall back to the stepwise runner otherwise.
`--wide-eval` scores a wider actor — the default 256 x 256 among them — in one launch as well, through the wide in-kernel
policy (`MLPPolicy.from_actor(actor, wide=True)`, include/salp_vec_policy_wide.h), and scores the kept checkpoint with the
stepwise runner too, so that the two success counts stand next to each other."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import underwater_swimmer_rl_amd as salp
from underwater_swimmer_rl_amd.navigation_eval import (pursuit_mlp, run_navigation_trials,
                                                       run_navigation_trials_in_kernel, summarize)
from underwater_swimmer_rl_amd.sac import SAC, DeviceReplayBuffer, SACConfig, train_sac_graphed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="single_food_long_horizon")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=30000, help="vector env steps")
    ap.add_argument("--segments", type=int, default=6)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--updates-per-step", type=int, default=2)
    ap.add_argument("--auto-alpha", action="store_true", help="learn the entropy coefficient (SB3's default) instead of the YAML's fixed alpha")
    ap.add_argument("--lr", type=float, default=None)
    ap.add_argument("--reward-scale", type=float, default=1.0, help="the learner sees reward * scale (the env's reward is unchanged)")
    ap.add_argument("--wide-eval", action="store_true",
                    help="score actors wider than 64 units (multiples of 32 up to 256) in one launch with the wide in-kernel policy")
    args = ap.parse_args()
    dev = "cuda:0"
    env = salp.SalpVectorEnv(args.preset, num_envs=args.envs, device=dev, seed=0)
    cfg = SACConfig.from_preset(args.preset)
    cfg.batch_size, cfg.updates_per_step, cfg.learning_starts = args.batch, args.updates_per_step, 200
    cfg.buffer_size = max(cfg.buffer_size, 200 * args.envs)
    if args.auto_alpha:
        cfg.alpha, cfg.target_entropy = None, None
    if args.lr:
        cfg.learning_rate = cfg.alpha_lr = args.lr
    agent = SAC(env.obs_dim, env.act_dim, cfg, device=dev, seed=0,
                act_low=env.single_action_space.low, act_high=env.single_action_space.high)

    def in_kernel_policy():
        """The actor's deterministic action as an in-kernel policy, or None when its shape does not fit one."""
        for wide in ((False, True) if args.wide_eval else (False,)):
            try:
                return salp.MLPPolicy.from_actor(agent.actor, wide=wide)
            except (ValueError, AttributeError):
                pass
        return None

    def evaluate(tag, heading_seed=0):
        # the whole trial loop in one kernel launch when the actor fits the in-kernel policy, else one launch per step
        mlp = in_kernel_policy()
        if mlp is not None:
            trials = run_navigation_trials_in_kernel(mlp, num_trials=100, device=dev, seed=123, heading_seed=heading_seed)
        else:
            pol = lambda o: agent.act(o, deterministic=True)
            trials = run_navigation_trials(pol, num_trials=100, device=dev, seed=123, heading_seed=heading_seed)
        m = summarize(trials)
        print(json.dumps({"eval": tag, **{k: round(float(v), 4) for k, v in m.items()}}), flush=True)
        return m

    scale = float(args.reward_scale)
    reward_fn = None if scale == 1.0 else (lambda o, a, r: r * scale)
    best, best_sd = -1.0, None

    print(json.dumps({"eval": "scripted pursuit baseline",
                      **{k: round(float(v), 4) for k, v in summarize(run_navigation_trials_in_kernel(pursuit_mlp(), num_trials=100, device=dev, seed=123)).items()}}), flush=True)
    evaluate("untrained policy")
    buf = DeviceReplayBuffer(cfg.buffer_size, env.obs_dim, env.act_dim, torch.device(dev))
    t0 = time.perf_counter()
    per = args.iters // args.segments
    for s in range(args.segments):
        env.clear_stats()
        m = train_sac_graphed(env, agent, per, buffer=buf, reward_fn=reward_fn)
        st = env.stats()
        print(json.dumps({"segment": s + 1, "wall_s": round(time.perf_counter() - t0, 1), "env_steps": st["env_steps"],
                          "food_per_1000_env_steps": round(1e3 * st["food_collected"] / max(st["env_steps"], 1), 4),
                          "episodes": st["episodes"], "critic_loss": round(m["critic_loss"], 4), "entropy": round(m["entropy"], 4)}), flush=True)
        e = evaluate(f"after segment {s + 1}")
        if e["success_rate"] > best:      # keep the best checkpoint, as a trainer's evaluation callback would
            best = e["success_rate"]
            best_sd = {k: (v.clone() if torch.is_tensor(v) else {kk: vv.clone() for kk, vv in v.items()}) for k, v in agent.state_dict().items()}
    if best_sd is not None:               # score the kept checkpoint on 100 trials with OTHER initial headings
        agent.load_state_dict(best_sd)
        m = evaluate("best checkpoint, fresh headings", heading_seed=7)
        if args.wide_eval:                # the same checkpoint and headings under the stepped protocol
            stepped = summarize(run_navigation_trials(lambda o: agent.act(o, deterministic=True), num_trials=100, device=dev, seed=123, heading_seed=7))
            print(json.dumps({"eval": "best checkpoint, fresh headings, one launch per step", "success_rate": round(float(stepped["success_rate"]), 4),
                              "same_success_count_as_one_launch": bool(round(100 * stepped["success_rate"]) == round(100 * m["success_rate"]))}), flush=True)
    env.close()


if __name__ == "__main__":
    main()
