#!/usr/bin/env python3
"""Wall time of the two navigation trial runners on one GPU: `run_navigation_trials` (one launch per env-step, positions read
back out of the float32 observation) and `run_navigation_trials_in_kernel` (salp_vec_evaluate_navigation: one launch).

Both are timed as a user calls them — env creation, set-up through set_state, the trial loop, the copies and the host metrics
— with a host clock around the whole call (each ends in device-to-host copies, so the device work is complete).  The share
spent in the host metrics (`navigation_metrics` / `metrics_from_record`, scipy splines included) is timed inside the same
call and reported next to the total.  Per shape: one warm-up call, then `--repeats` timed calls, the median and the spread.
Also prints the four navigation kernels' resources from salp_vec_last_kernel_resources.

    python profiles/navigation_wall.py --trials 256 --steps 3000 --repeats 5 --out navigation_wall.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed_runner(ne, which, n, steps, track):
    """One call of a runner; returns (total seconds, seconds inside the host metrics, summary)."""
    import torch
    spent = [0.0]

    def wrap(fn):
        def inner(*a, **k):
            t0 = time.perf_counter()
            out = fn(*a, **k)
            spent[0] += time.perf_counter() - t0
            return out
        return inner

    keep = ne.navigation_metrics, ne.metrics_from_record
    ne.navigation_metrics, ne.metrics_from_record = wrap(keep[0]), wrap(keep[1])
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if which == "stepwise":
            m = ne.run_navigation_trials(ne.pursuit_policy(), num_trials=n, max_steps=steps, seed=3, heading_seed=1)
        else:
            m = ne.run_navigation_trials_in_kernel(ne.pursuit_mlp(), num_trials=n, max_steps=steps, seed=3, heading_seed=1, track=track)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    finally:
        ne.navigation_metrics, ne.metrics_from_record = keep
    s = ne.summarize(m)
    return total, spent[0], dict(success_rate=s["success_rate"], avg_steps=s["avg_steps"], avg_path_ratio=s["avg_path_ratio"])


def kernel_resources():
    from underwater_swimmer_rl_amd import SalpVectorEnv
    from underwater_swimmer_rl_amd.navigation_eval import navigation_config, pursuit_mlp
    out = {}
    for width, consts in ((800, "literal"), (900, "run-time")):
        for n, form in ((128, "unpredicated"), (100, "predicated")):
            env = SalpVectorEnv(navigation_config(width=width), n, device="cuda:0", seed=0)
            env.reset()
            env.evaluate_navigation(pursuit_mlp(), 4, (150.0, 300.0, 650.0, 300.0))
            ll = env._lib.last_launch()
            assert ll["full_signature"] == 5 and (ll["envs_predicated"] > 0) == (form == "predicated")
            out[f"{consts} constants, {form}"] = env._lib.last_kernel_resources()
            env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, nargs="+", default=[256])
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runners", nargs="+", default=["stepwise", "in_kernel", "in_kernel_no_track"])
    ap.add_argument("--no-warmup", action="store_true", help="the shape's kernels are warm already (an earlier shape of this run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured (this script has no CPU fallback)")
    from underwater_swimmer_rl_amd import navigation_eval as ne
    res = dict(device=torch.cuda.get_device_name(0), steps=a.steps, repeats=a.repeats, kernels=kernel_resources(), shapes=[])
    print(json.dumps(dict(kernels=res["kernels"])), flush=True)
    for n in a.trials:
        for runner in a.runners:
            which, track = ("stepwise", True) if runner == "stepwise" else ("in_kernel", runner == "in_kernel")
            if not a.no_warmup:
                timed_runner(ne, which, n, a.steps, track)
            runs = []
            for _ in range(a.repeats):
                runs.append(timed_runner(ne, which, n, a.steps, track))
                print(f"  {runner} n={n}: {runs[-1][0]:.4f} s (host metrics {runs[-1][1]:.4f} s)", flush=True)
            tot = [r[0] for r in runs]
            row = dict(runner=runner, trials=n, median_s=statistics.median(tot), min_s=min(tot), max_s=max(tot),
                       median_host_metrics_s=statistics.median(r[1] for r in runs), summary=runs[-1][2], warmup=not a.no_warmup)
            res["shapes"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
