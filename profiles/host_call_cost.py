#!/usr/bin/env python3
"""Host cost of one device-pointer salp_vec_step in the launch-bound case (64 envs by default): what the C ABI's own code
adds on top of the launch, for several builds of libsalp_hip.so alternating in ONE process.  usage:
    python profiles/host_call_cost.py name1=path1.so name2=path2.so ... [--envs 64] [--rounds 40] [--calls 200]
A sample is the host wall time of `calls` consecutive calls (nothing waits for the GPU inside it; the stream is drained
between samples, outside the clock) divided by `calls`.  Prints per variant the median, mean, min and max over the rounds."""
import ctypes, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import underwater_swimmer_rl_amd as pkg
from underwater_swimmer_rl_amd import _capi


def main():
    variants, n, rounds, calls = [], 64, 40, 200
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--envs": n = int(next(it))
        elif a == "--rounds": rounds = int(next(it))
        elif a == "--calls": calls = int(next(it))
        else:
            k, v = a.split("=", 1); variants.append((k, os.path.abspath(v)))
    cfg = pkg.load_env_config("single_food_long_horizon")
    dev = torch.device("cuda", 0)
    act = torch.rand((n, cfg.act_dim), device=dev) * 2 - 1
    obs = torch.empty((n, cfg.obs_dim), device=dev)
    rew = torch.empty((n,), device=dev)
    term = torch.empty((n,), dtype=torch.uint8, device=dev)
    trunc = torch.empty((n,), dtype=torch.uint8, device=dev)
    vp = ctypes.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    steps = {}
    for name, path in variants:
        lib = _capi.load_library(path)
        c, h = cfg.to_c(), ctypes.c_void_p()
        _capi.check(lib, lib.salp_vec_create(ctypes.byref(c), n, 0, 0, 0, ctypes.byref(h)), "create")
        args = (h, vp(act.data_ptr()), vp(obs.data_ptr()), vp(rew.data_ptr()), vp(term.data_ptr()), vp(trunc.data_ptr()), None, None,
                _capi.SALP_DEVICE_PTRS, st)
        steps[name] = (lib, lib.salp_vec_step, args)
    times = {name: [] for name, _ in variants}
    for r in range(rounds + 2):                     # the first two rounds warm up
        for name, _ in variants:
            lib, step, args = steps[name]
            t0 = time.perf_counter()
            for _ in range(calls):
                rc = step(*args)
            dt = time.perf_counter() - t0
            _capi.check(lib, rc, "step")
            torch.cuda.synchronize()
            if r >= 2:
                times[name].append(dt / calls * 1e6)
    print(json.dumps({name: {"median_us": round(statistics.median(t), 3), "mean_us": round(statistics.fmean(t), 3), "min_us": round(min(t), 3),
                             "max_us": round(max(t), 3), "rounds": len(t), "calls_per_round": calls, "envs": n} for name, t in times.items()}, indent=1))


if __name__ == "__main__":
    main()
