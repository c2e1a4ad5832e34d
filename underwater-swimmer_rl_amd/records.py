"""The packed transition record of `salp_vec_step_packed` / `salp_vec_rollout_packed` (include/salp_vec.h "Packed
transition record"): one row of 32-bit words per env and step,

    [ obs (obs_dim float32) | reward float32 | flags word | food_collected int32 | steps_since_food int32 | final obs ]

flags word: byte 0 terminated, byte 1 truncated, byte 2 collision, byte 3 zero.  The terminal-observation tail (obs_dim more
float32) is there when the block was asked for with it; rows of unfinished envs leave it unwritten.  Integers are stored as
integers, so every field is a typed VIEW of the block: `unpack_record` copies nothing, for numpy arrays and torch tensors
(CPU or GPU) alike.  `pack_record` is the numpy restatement of the layout, for tests and CPU engines.
"""
from __future__ import annotations

import numpy as np

REC_REWARD, REC_FLAGS, REC_FOOD_COLLECTED, REC_STEPS_SINCE_FOOD, REC_EXTRA_COLS = range(5)   # _capi.REC_* / SALP_REC_*


def record_width(obs_dim: int, with_final: bool) -> int:
    """Words per record: obs_dim + 4, or 2 obs_dim + 4 with the terminal observation."""
    return int(obs_dim) + REC_EXTRA_COLS + (int(obs_dim) if with_final else 0)


def _has_final(width: int, obs_dim: int) -> bool:
    if width == record_width(obs_dim, False):
        return False
    if width == record_width(obs_dim, True):
        return True
    raise ValueError(f"a record of obs_dim {obs_dim} is {record_width(obs_dim, False)} or {record_width(obs_dim, True)} "
                     f"words wide, not {width}")


def unpack_record(rec, obs_dim: int) -> dict:
    """Zero-copy views of a float32 record block [..., width]: obs [..., obs_dim] and reward [...] float32, terminated /
    truncated [...] bool, collision [...] uint8, food_collected / steps_since_food [...] int32, final_observation
    [..., obs_dim] float32 or None when the width says the block has no tail."""
    D = int(obs_dim)
    with_final = _has_final(int(rec.shape[-1]), D)
    if isinstance(rec, np.ndarray):
        if rec.dtype != np.float32:
            raise TypeError("record blocks are float32")
        words, u8, boolean = rec.view(np.int32), rec.view(np.uint8), np.bool_
    else:                                   # torch tensor
        import torch
        if rec.dtype != torch.float32:
            raise TypeError("record blocks are float32")
        words, u8, boolean = rec.view(torch.int32), rec.view(torch.uint8), torch.bool
    fb = 4 * (D + REC_FLAGS)                # byte offset of the flags word in a row
    return {
        "obs": rec[..., :D],
        "reward": rec[..., D + REC_REWARD],
        "terminated": u8[..., fb].view(boolean),
        "truncated": u8[..., fb + 1].view(boolean),
        "collision": u8[..., fb + 2],
        "food_collected": words[..., D + REC_FOOD_COLLECTED],
        "steps_since_food": words[..., D + REC_STEPS_SINCE_FOOD],
        "final_observation": rec[..., D + REC_EXTRA_COLS:] if with_final else None,
    }


def transitions(first_obs, record, actions, obs_dim: int):
    """The replay tuples of a closed-loop block (`SalpVectorEnv.rollout_policy_packed`, records with the terminal tail):
    `(obs, actions, reward, next_obs, terminated)` over all H x N rows, flattened to [H * N, ...] in step order.
      obs       the row each action saw: `first_obs` [N, obs_dim] (the observation before the call), then the record's obs
                of step t - 1 — one new [H, N, obs_dim] block;
      next_obs  the terminal tail where the row is finished (terminated | truncated), else the record's obs (after the
                same-step autoreset the record's obs of a finished row is the next episode's first row).  The tails of
                unfinished rows — never written by the kernels — are selected around, not multiplied: nothing of them,
                a NaN included, reaches the result;
      actions, reward, terminated   views of `actions` and of the block (no copy).
    numpy arrays and torch tensors (CPU or GPU) alike, like `unpack_record`."""
    D = int(obs_dim)
    f = unpack_record(record, D)
    if f["final_observation"] is None:
        raise ValueError("transitions needs records with the terminal observation (want_final_observation=True)")
    if record.ndim != 3:
        raise ValueError(f"a record block is [H, N, width]; got {tuple(record.shape)}")
    H, N = int(record.shape[0]), int(record.shape[1])
    if tuple(first_obs.shape) != (N, D) or tuple(actions.shape[:2]) != (H, N):
        raise ValueError(f"first_obs {tuple(first_obs.shape)} / actions {tuple(actions.shape)} do not fit a block of {H} x {N} rows of obs_dim {D}")
    if isinstance(record, np.ndarray):
        seen = np.empty((H, N, D), np.float32)
        done = np.logical_or(f["terminated"], f["truncated"])
        next_obs = np.where(done[..., None], f["final_observation"], f["obs"])
    else:
        import torch
        seen = torch.empty((H, N, D), dtype=torch.float32, device=record.device)
        done = torch.logical_or(f["terminated"], f["truncated"])
        next_obs = torch.where(done[..., None], f["final_observation"], f["obs"])
    seen[0] = first_obs
    seen[1:] = f["obs"][:-1]
    flat = lambda t: t.reshape((H * N,) + tuple(t.shape[2:]))
    return flat(seen), flat(actions), f["reward"].reshape(H * N), flat(next_obs), f["terminated"].reshape(H * N)


def pack_record(obs, reward, terminated, truncated, info, final_obs=None) -> np.ndarray:
    """The layout in numpy: obs [..., D], reward / terminated / truncated [...], info [..., 3] int (food_collected,
    steps_since_food, collision: the SALP_INFO_* columns), final_obs [..., D] or None -> float32 [..., width].  The whole
    of `final_obs` is copied (a caller that wants unfinished rows untouched overwrites only the rows it needs)."""
    obs = np.asarray(obs, dtype=np.float32)
    D = obs.shape[-1]
    info = np.asarray(info)
    rec = np.zeros(obs.shape[:-1] + (record_width(D, final_obs is not None),), np.float32)
    rec[..., :D] = obs
    rec[..., D + REC_REWARD] = np.asarray(reward, dtype=np.float32)
    words = rec.view(np.uint32)
    words[..., D + REC_FLAGS] = ((np.asarray(terminated) != 0).astype(np.uint32)
                                 | ((np.asarray(truncated) != 0).astype(np.uint32) << 8)
                                 | ((info[..., 2] != 0).astype(np.uint32) << 16))
    ints = rec.view(np.int32)
    ints[..., D + REC_FOOD_COLLECTED] = info[..., 0]
    ints[..., D + REC_STEPS_SINCE_FOOD] = info[..., 1]
    if final_obs is not None:
        rec[..., D + REC_EXTRA_COLS:] = np.asarray(final_obs, dtype=np.float32)
    return rec
