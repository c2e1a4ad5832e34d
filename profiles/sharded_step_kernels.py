#!/usr/bin/env python3
"""ShardedSalpVectorEnv.step at RCCL world size 1, for a kernel trace (kernels per step around the
collective).  usage, one mode per run, nothing else traced in the same run:
    rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python profiles/sharded_step_kernels.py packed|unpacked [steps] [envs]
`unpacked` hides the engine's step_packed, which is the path every engine took before the packed record existed."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.distributed as dist
from underwater_swimmer_rl_amd.sharded import ShardedSalpVectorEnv


class Unpacked:
    """The engine without step_packed."""
    def __init__(self, engine): self._e = engine
    def step(self, a): return self._e.step(a)
    def reset(self, **kw): return self._e.reset(**kw)
    def close(self): self._e.close()


def main():
    mode = sys.argv[1]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 131072
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29551")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        env = ShardedSalpVectorEnv("sac_gail", n, device="cuda:0", seed=0)
        if mode == "unpacked":
            env.engine = Unpacked(env.engine)
        a = torch.rand((n, env.act_dim), device=env.device) * 2 - 1
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(steps):
            env.step(a)
        e.record(); e.synchronize()
        print(f"{mode}: {steps} steps of {n} envs, {s.elapsed_time(e) / steps * 1e3:.1f} us per step")
        env.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
