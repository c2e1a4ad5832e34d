#!/usr/bin/env python3
"""Cost of recording cycle histories (salp_robot_step_record_kernel, salp_robot_vec_step_history) against the plain
step (salp_robot_step_kernel): ms per batch of breathing cycles and the history bytes written per ms, as a share of
the 6.29 TB/s copy ceiling of MI355X_MICROARCH.md.  One JSON line per (coast, mode).
    python profiles/robot_history_perf.py [--envs N] [--iters K]
    python profiles/robot_history_perf.py --layouts     # store-layout experiment, schedule off (below)
Timed with events around env.step after one warm-up step; confirm with a rocprofv3 --kernel-trace --stats run.

--layouts builds (if not current) the experiment libraries of salp_robot.hip under profiles/variants/ and times every
env at stride 1 and 10 with the longest-cycle-first schedule off, one child process per library: env-major [rec][cap][16]
or time-major [cap][16][rec] (-DSALP_ROBOT_HIST_TIME_MAJOR), temporal or non-temporal stores (-DSALP_ROBOT_HIST_NONTEMPORAL);
the product library is env-major with temporal stores.
The time-major libraries write that layout into the same buffer; only the timing of their output is meaningful."""
import argparse
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from underwater_swimmer_rl_amd.robot_env import H_COUNT, SalpRobotVectorEnv  # noqa: E402

COPY_CEILING_GBS = 6290.0
VARIANTS = {"env_major_temporal": (), "env_major_nontemporal": ("SALP_ROBOT_HIST_NONTEMPORAL",),
            "time_major_temporal": ("SALP_ROBOT_HIST_TIME_MAJOR",),
            "time_major_nontemporal": ("SALP_ROBOT_HIST_TIME_MAJOR", "SALP_ROBOT_HIST_NONTEMPORAL")}


def variant_library(name):
    spec = importlib.util.spec_from_file_location("_salp_build", os.path.join(ROOT, "underwater-swimmer_rl_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    if not VARIANTS[name]:
        return b.build()
    return b.build(out=os.path.join(ROOT, "profiles", "variants", f"libsalp_hist_{name}.so"), defines=VARIANTS[name])


def run(n, coast_hi, mode, iters):
    env = SalpRobotVectorEnv(n, device="cuda:0", seed=0)
    if mode is not None:
        env.record_history(mode[0], stride=mode[1])
    g = torch.Generator(device="cuda").manual_seed(0)

    def actions():
        a = torch.rand((n, 3), generator=g, device="cuda")
        a[:, 1] *= coast_hi
        a[:, 2] = a[:, 2] * 2 - 1
        return a
    env.step(actions())
    torch.cuda.synchronize()
    tot_ms, samples, inner = 0.0, 0, 0
    for _ in range(iters):
        a = actions()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        obs, rew, term, trunc, info = env.step(a)
        e.record()
        e.synchronize()
        tot_ms += s.elapsed_time(e)
        inner += int(info["inner_steps"].sum())
        if mode is not None:
            samples += int(info["cycle_history_len"].sum())
    rec = 0 if mode is None else env._hist[1]
    env.close()
    ms = tot_ms / iters
    gb = samples * H_COUNT * 4 / iters / 1e9
    return {"envs": n, "coast_max_s": 10 * coast_hi, "recorded_envs": rec, "stride": None if mode is None else mode[1],
            "ms_per_batch": round(ms, 4), "mean_inner_steps": inner / (n * iters), "history_GB_per_batch": round(gb, 4),
            "history_GB_per_s": round(gb / (ms / 1e3), 1), "share_of_copy_ceiling": round(gb / (ms / 1e3) / COPY_CEILING_GBS, 4)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=262144)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layouts", action="store_true")
    ap.add_argument("--variant", default=None)      # child of --layouts
    args = ap.parse_args()
    if args.layouts:
        for name in VARIANTS:
            env = dict(os.environ, SALP_HIP_LIBRARY=variant_library(name), SALP_ROBOT_SCHEDULE="0")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", name, "--envs", str(args.envs),
                            "--iters", str(args.iters)], env=env, check=True)
    elif args.variant:
        for coast_hi in (0.1, 1.0):
            for mode in ((None, 1), (None, 10)):
                print(json.dumps({"variant": args.variant, "schedule": 0, "coast_hi": coast_hi,
                                  **run(args.envs, coast_hi, mode, args.iters)}), flush=True)
    else:
        for coast_hi in (0.1, 1.0):
            for mode in (None, (slice(0, 1024), 1), (None, 1), (None, 10)):
                print(json.dumps({"coast_hi": coast_hi, **run(args.envs, coast_hi, mode, args.iters)}), flush=True)
