"""Host-side mirror of the reference interface: parameters, spaces, SB3 adapter plumbing, bench maths."""
import math
import os
import sys

import numpy as np
import pytest

import underwater_swimmer_rl_amd as pkg
from underwater_swimmer_rl_amd import spaces
from underwater_swimmer_rl_amd.vector_env import _LazyInfos

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_defaults_are_the_reference_kwargs():
    c = pkg.SalpSnakeConfig()
    # snake:29-33
    assert (c.width, c.height, c.num_food_items, c.food_reward, c.collision_penalty) == (800, 600, 5, 10.0, -50.0)
    assert (c.time_penalty, c.efficiency_bonus, c.forced_breathing, c.max_observed_food) == (-0.1, 1.0, True, 3)
    assert (c.random_food_count, c.respawn_food, c.proximity_reward_weight, c.max_steps_without_food) == (False, True, 0.0, 1500)
    # legacy:32-53
    assert (c.tank_margin, c.base_radius, c.max_thrust_force, c.drag_coefficient) == (50.0, 30.0, 100.0, 0.98)
    assert c.max_nozzle_angle == math.pi / 3 and c.nozzle_response_rate == 0.05
    assert (c.inhale_duration, c.exhale_duration, c.rest_duration) == (120, 150, 60)
    assert c.obs_dim == 24 and c.act_dim == 1


def test_presets_and_overrides():
    c = pkg.load_env_config("single_food_long_horizon")
    assert c.collision_penalty == -500.0 and c.max_steps_without_food == 2000 and c.num_food_items == 1
    assert pkg.load_env_config("sac_gail").num_food_items == 12
    assert pkg.load_env_config("single_food", forced_breathing=False).act_dim == 2
    assert pkg.SalpSnakeConfig(num_food_items=-3).num_food_items == 0       # snake:36 max(0, n)
    with pytest.raises(TypeError):
        pkg.load_env_config("single_food", not_a_param=1)
    with pytest.raises(ValueError):
        pkg.SalpSnakeConfig(num_food_items=17)
    with pytest.raises(FileNotFoundError):
        pkg.load_env_config("no_such_preset")


def test_yaml_loader(tmp_path):
    p = tmp_path / "x.yaml"
    p.write_text("environment:\n  width: 999\n  params:\n    num_food_items: 2\n    food_reward: 3.5\n")
    c = pkg.load_env_config(str(p))
    assert c.num_food_items == 2 and c.food_reward == 3.5 and c.width == 800  # train.py:50-52 drops width/height


def test_spaces_match_snake_69_88():
    cfg = pkg.load_env_config("single_food")
    a, o = spaces.single_action_space(cfg), spaces.single_observation_space(cfg)
    assert a.shape == (1,) and a.low[0] == -1 and a.high[0] == 1 and a.dtype == np.float32
    assert o.shape == (24,) and o.low[4] == np.float32(-math.pi) and o.high[6] == 2.0 and o.low[10] == -1
    a2 = spaces.single_action_space(pkg.load_env_config("single_food", forced_breathing=False))
    assert a2.shape == (2,) and list(a2.low) == [0.0, -1.0] and list(a2.high) == [1.0, 1.0]
    b = spaces.batch_space(o, 7)
    assert b.shape == (7, 24) and a.contains(a.sample())


def test_lazy_infos_behave_like_a_list_of_dicts():
    n = 5
    dones = np.array([0, 1, 0, 1, 0], bool)
    truncs = np.array([0, 1, 0, 0, 0], bool)
    tobs = np.arange(n * 3, dtype=np.float32).reshape(n, 3)
    inf = _LazyInfos(n, np.arange(n), np.arange(n) * 2, np.zeros(n, np.int32), dones, truncs, tobs, 10.0)
    assert len(inf) == n and inf[1]["TimeLimit.truncated"] and not inf[3]["TimeLimit.truncated"]
    assert "terminal_observation" in inf[3] and "terminal_observation" not in inf[0]
    assert inf[-1]["food_collected"] == 4 and inf[2]["score"] == 20.0 and len(inf[1:3]) == 2


def test_bench_roofline_accounting():
    sys.path.insert(0, ROOT)
    import bench
    cfg = pkg.load_env_config("single_food_long_horizon")
    assert bench.algorithmic_bytes_per_env_step(cfg, 1) == 218.0              # SURVEY.md §8d step-per-launch
    assert abs(bench.algorithmic_bytes_per_env_step(cfg, 5000) - 106.0224) < 1e-9
    assert bench.algorithmic_bytes_per_env_step(pkg.load_env_config("sac_gail"), 1) == 394.0


def test_bench_shard_plan_is_baseline_configs_2_and_3():
    """bench.py --gpus 1 measures BASELINE configs[2] (262144 envs), --gpus G > 1 configs[3]: 1 048 576 envs in total,
    split by contiguous env-index blocks (131072 per GPU at G = 8, env_index_base = rank * 131072)."""
    import bench
    p1 = bench.shard_plan(1)
    assert (p1["envs_per_gpu"], p1["total_envs"], p1["config"], p1["scaling"]) == (262144, 262144, 2, "weak")
    for g, per in ((2, 524288), (4, 262144), (8, 131072)):
        p = bench.shard_plan(g)
        assert (p["envs_per_gpu"], p["total_envs"], p["config"], p["scaling"]) == (per, 1048576, 3, "strong")
        assert [p["env_index_base"](r) for r in range(g)] == [r * per for r in range(g)]
    pw = bench.shard_plan(8, weak=True)
    assert (pw["envs_per_gpu"], pw["total_envs"], pw["config"], pw["scaling"]) == (262144, 8 * 262144, 2, "weak")
    assert bench.shard_plan(2, total_envs=32768)["config"] is None          # an override is labelled as such
    with pytest.raises(ValueError):
        bench.shard_plan(3)                                                   # 1048576 does not split over 3 ranks
    with pytest.raises(ValueError):
        bench.shard_plan(2, envs_per_gpu=8, total_envs=16)


def test_bench_dump_outputs_is_a_seeded_float32_sample(tmp_path):
    """bench.py --dump-outputs: the same seeded env sample every run, float32 files, flags as 0 / 1."""
    import torch
    import bench
    H, n, D = 3, 5000, 24
    g = torch.Generator().manual_seed(0)
    res = dict(obs=torch.rand((H, n, D), generator=g), reward=torch.rand((H, n), generator=g),
               terminated=(torch.rand((H, n), generator=g) < 0.1).to(torch.uint8),
               truncated=(torch.rand((H, n), generator=g) < 0.1).to(torch.uint8), final_obs=None, actions=None)
    files = bench.dump_outputs(str(tmp_path / "a"), res, n, generated_actions=False)
    bench.dump_outputs(str(tmp_path / "b"), res, n, generated_actions=False)
    assert sorted(files) == ["env_index.npy", "obs.npy", "reward.npy", "terminated.npy", "truncated.npy"]
    idx = np.load(tmp_path / "a" / "env_index.npy")
    assert idx.dtype == np.float64 and len(idx) == bench.DUMP_ENVS and len(np.unique(idx)) == bench.DUMP_ENVS
    ii = idx.astype(np.int64)
    for name in files:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert np.array_equal(a, b) and a.dtype in (np.float32, np.float64), name
        if name != "env_index.npy":
            assert a.dtype == np.float32 and np.array_equal(a, res[name[:-4]][:, ii].numpy().astype(np.float32)), name
    assert bench.DUMP_ENVS * 250 * (D + 3) * 4 <= bench.DUMP_BYTES < 64 * 10**6  # the bench's default chunk: DUMP_ENVS envs


def test_bench_dump_outputs_stays_within_its_byte_budget(tmp_path, monkeypatch):
    """A longer chunk gets fewer envs, one that a single env cannot fit only its last steps: never more than DUMP_BYTES."""
    import torch
    import bench
    H, n, D = 40, 300, 24
    g = torch.Generator().manual_seed(1)
    res = dict(obs=torch.rand((H, n, D), generator=g), reward=torch.rand((H, n), generator=g),
               terminated=torch.zeros((H, n), dtype=torch.uint8), truncated=torch.ones((H, n), dtype=torch.uint8),
               actions=torch.rand((H, n, 2), generator=g))
    for budget, envs, steps in ((10**9, 300, H), (100_000, 100_000 // (H * 29 * 4 + 8), H), (2_000, 1, (2_000 - 8) // (29 * 4))):
        monkeypatch.setattr(bench, "DUMP_BYTES", budget)
        out = tmp_path / str(budget)
        files = bench.dump_outputs(str(out), res, n, generated_actions=True)
        arrays = {f[:-4]: np.load(out / f) for f in files}
        assert sum(a.nbytes for a in arrays.values()) <= budget
        ii = arrays["env_index"].astype(np.int64)
        assert len(ii) == envs and arrays["obs"].shape == (steps, envs, D) and arrays["actions"].shape == (steps, envs, 2)
        for name in ("obs", "reward", "terminated", "truncated", "actions"):
            assert np.array_equal(arrays[name], res[name][H - steps:][:, ii].numpy().astype(np.float32)), name


def test_adaptive_food_curriculum_follows_the_reference_rule():
    """continuous_trainer.py:375-415: window of 10 episodes, > 0.6 removes a food, < 0.25 adds one, within [2, 12],
    window cleared after a change; the change is the base_num_food_items write."""
    from underwater_swimmer_rl_amd.curriculum import AdaptiveFoodCurriculum

    class Env:
        base_num_food_items = 5

    env = Env()
    cur = AdaptiveFoodCurriculum(env)
    for _ in range(9):
        assert not cur.record_episode(5, 5)            # window not full yet
    assert cur.record_episode(5, 5) and env.base_num_food_items == 4 and cur.recent_food_collection_rates == []
    for _ in range(9):
        assert not cur.record_episode(0, 4)
    assert cur.record_episode(0, 4) and env.base_num_food_items == 5
    for _ in range(30):                                # middling performance: nothing changes, the window slides
        assert not cur.record_episode(2, 5)
    assert len(cur.recent_food_collection_rates) == 10 and env.base_num_food_items == 5
    env.base_num_food_items = 2
    low = AdaptiveFoodCurriculum(env)
    assert low.record_finished([2] * 25, [2] * 25) == 0 and env.base_num_food_items == 2      # floor
    env.base_num_food_items = 12
    high = AdaptiveFoodCurriculum(env)
    assert high.record_finished([0] * 25, [12] * 25) == 0 and env.base_num_food_items == 12   # ceiling
    assert cur.changes == [4, 5]
