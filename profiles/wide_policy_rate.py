#!/usr/bin/env python3
"""Rate of the wide in-kernel policy (include/salp_vec_policy_wide.h) against the route the project offered before for the
same actor.  Needs an MI355X.  usage:  python profiles/wide_policy_rate.py [--out profiles/wide_policy_rate.json]

The actor is `sac.Actor(24, 1)` with its default hidden sizes (256, 256), freshly initialised (seed 0): the rate does not
depend on the weights.  Per size (4096, 65536, 262144 envs; H = 64 steps per call):
  wide      `SalpVectorEnv.evaluate_policy(handle, 64)` with `MLPPolicy.from_actor(actor, wide=True)`: one launch, no per-step
            output;
  baseline  `SalpVectorEnv.capture_policy_steps(actor's deterministic forward, 64)`: one hipGraph of 64 x (torch forward,
            salp_vec_step), replayed.
Both run in one process on twin envs, alternating, each call ended by a device synchronise under a host clock; after two
warm-up pairs the medians of PAIRS pairs are reported as env-steps per second, with their ratio and the wide rate as a
fraction of the derived ceiling: 2496 v_mfma_f32_32x32x2_f32 per wavefront-step (layer 0: 192, layer 1: 2048, last layer: 256)
at 64 cycles each, on 1024 SIMDs at 2.4 GHz = 9.85e8 env-steps/s."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, PAIRS, WARMUP = 64, 7, 2
SIZES = (4096, 65536, 262144)
MFMA_PER_WAVE_STEP = 2 * (8 * 12 + 8 * 128 + 8 * 16)          # two env halves; 8 tiles of 12, 128 and 16 k-steps
CEILING = 1024 * 64 * 2.4e9 / (MFMA_PER_WAVE_STEP * 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "wide_policy_rate.json"))
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    args = ap.parse_args()
    import torch
    import underwater_swimmer_rl_amd as salp
    from underwater_swimmer_rl_amd import sac
    assert MFMA_PER_WAVE_STEP == 2496
    torch.manual_seed(0)
    actor = sac.Actor(24, 1).to("cuda:0")
    policy = salp.MLPPolicy.from_actor(actor, wide=True)
    forward = lambda o: actor(o, deterministic=True, with_logprob=False)[0]
    rows = []
    for n in args.sizes:
        env_w = salp.SalpVectorEnv("single_food", num_envs=n, device="cuda:0", seed=0)
        env_b = salp.SalpVectorEnv("single_food", num_envs=n, device="cuda:0", seed=0)
        env_w.reset()
        env_b.reset()
        handle = env_w.make_policy(policy)
        with torch.no_grad():
            graph = env_b.capture_policy_steps(forward, H, want_final_observation=False)

        def timed(call):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        tw, tb = [], []
        for k in range(WARMUP + PAIRS):
            a = timed(lambda: env_w.evaluate_policy(handle, H))
            b = timed(graph.replay)
            if k >= WARMUP:
                tw.append(a)
                tb.append(b)
        assert env_w._lib.last_launch_policy_wide() == 1
        res = env_w._lib.last_kernel_resources()
        w, b = n * H / statistics.median(tw), n * H / statistics.median(tb)
        row = dict(envs=n, horizon=H, pairs=PAIRS, wide_env_steps_per_s=w, baseline_env_steps_per_s=b, ratio=w / b,
                   fraction_of_ceiling=w / CEILING, wide_seconds=sorted(tw), baseline_seconds=sorted(tb), kernel=res)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del graph
        handle.close()
        env_w.close()
        env_b.close()
    with open(args.out, "w") as f:
        json.dump(dict(actor="24-256-256-1, tanh", mfma_per_wavefront_step=MFMA_PER_WAVE_STEP, ceiling_env_steps_per_s=CEILING, rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
