"""The paths of the Python shim (vector_env.py, robot_env.py over _arrays.py and _capi.py) that fork on what the caller
hands in: the action fast path of `step` / `step_packed` against the converting path, the handle cache of a policy object,
the refusals of an evaluation's `out` block and the forms of a reset mask.  Run with `pytest -m gpu`.

96 envs (one full wavefront and a ragged 32), 3 steps, the navigation config (one food, forced breathing, no_autoreset,
K = 3), so that one env serves every policy call.  Envs of equal seed are compared bit for bit."""
import numpy as np
import pytest

from underwater_swimmer_rl_amd.navigation_eval import navigation_config, pursuit_mlp
from underwater_swimmer_rl_amd.policy import EVAL_WORDS, NAV_WORDS
from underwater_swimmer_rl_amd.records import unpack_record
from underwater_swimmer_rl_amd.robot_env import SalpRobotVectorEnv
from underwater_swimmer_rl_amd.vector_env import SalpVectorEnv

pytestmark = pytest.mark.gpu

N, H, SEED = 96, 3, 5
LINE = (400.0, 300.0, 500.0, 300.0)
MASK = (np.arange(N) % 3 != 1) | (np.arange(N) >= 64)          # ragged, in both wavefronts


def snake(output="torch"):
    return SalpVectorEnv(navigation_config(), N, device="cuda:0", seed=SEED, output=output)


def host(x):
    """Any output (tensor, array, None) as a host array of bytes-comparable content."""
    return None if x is None else np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x)


def same(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def action_forms(output, a32):
    """float32 [N, A] actions in the forms that take different routes into the kernel; form 0 is the direct one."""
    strided = np.zeros((N, 2 * a32.shape[1]), np.float32)
    strided[:, ::2] = a32
    if output == "numpy":
        return [a32, a32.astype(np.float64).tolist(), strided[:, ::2]]
    import torch
    dev = torch.from_numpy(a32).to("cuda:0")
    far = torch.from_numpy(strided).to("cuda:0")[:, ::2]
    assert dev.is_contiguous() and dev.dtype == torch.float32 and not far.is_contiguous()
    return [dev, a32.astype(np.float64), far]


@pytest.mark.parametrize("output", ["torch", "numpy"])
def test_step_fast_path_equals_the_converting_path(output):
    envs = [snake(output) for _ in range(3)]
    for e in envs:
        e.reset()
    rng = np.random.default_rng(0)
    for t in range(H):
        a32 = rng.uniform(-1, 1, (N, envs[0].act_dim)).astype(np.float32)
        outs = [e.step(a) for e, a in zip(envs, action_forms(output, a32))]
        assert outs[0][0] is envs[0]._step_cache["obs"] and outs[0][0] is envs[0]._bufs["obs"]      # the env's own buffers
        for k in (1, 2):
            for j in range(4):
                assert same(outs[0][j], outs[k][j]), (t, k, j)
            i0, ik = outs[0][4], outs[k][4]
            assert sorted(i0) == sorted(ik) == ["_final_observation", "collision", "final_observation", "food_collected",
                                                "steps_since_food"]
            for key in ("food_collected", "steps_since_food", "collision", "_final_observation"):
                assert same(i0[key], ik[key]), (t, k, key)
            done = host(i0["_final_observation"])
            assert np.array_equal(done, host(outs[0][2]) | host(outs[0][3]))
            assert same(host(i0["final_observation"])[done], host(ik["final_observation"])[done])
    for e in envs:
        e.close()


@pytest.mark.parametrize("with_final", [False, True])
@pytest.mark.parametrize("output", ["torch", "numpy"])
def test_step_packed_fast_path_equals_the_converting_path(output, with_final):
    envs = [snake(output) for _ in range(3)]
    for e in envs:
        e.reset()
    rng = np.random.default_rng(1)
    D = envs[0].obs_dim
    for t in range(H):
        a32 = rng.uniform(-1, 1, (N, envs[0].act_dim)).astype(np.float32)
        recs = [host(e.step_packed(a, want_final_observation=with_final)) for e, a in zip(envs, action_forms(output, a32))]
        assert recs[0].shape == (N, (2 * D if with_final else D) + 4)
        u = unpack_record(recs[0], D)
        done = u["terminated"] | u["truncated"]
        for k in (1, 2):
            assert same(recs[0][:, :D + 4], recs[k][:, :D + 4]), (t, k)
            assert same(recs[0][done, D + 4:], recs[k][done, D + 4:]), (t, k)      # the tail of an unfinished row is not written
    # the packed record holds what step returns
    plain = snake(output)
    plain.reset()
    rng = np.random.default_rng(1)
    for t in range(H):
        obs, rew, term, trunc, info = plain.step(rng.uniform(-1, 1, (N, plain.act_dim)).astype(np.float32))
    assert same(obs, u["obs"]) and same(rew, u["reward"]) and same(term, u["terminated"]) and same(trunc, u["truncated"])
    for e in envs + [plain]:
        e.close()


def test_one_policy_object_gets_one_handle_and_close_resets_the_caches():
    import torch
    env = snake()
    env.reset()
    policy = pursuit_mlp(3.0)
    assert env._lib._policies == [] and env._policy_cache == {} and env._step_cache is None and env._packed_cache == {}
    r = env.rollout_policy(policy, H)
    ev = env.evaluate_policy(policy, H)
    nav = env.evaluate_navigation(policy, H, LINE)
    torch.cuda.synchronize()
    assert len(env._lib._policies) == 1 and list(env._policy_cache) == [id(policy)]
    assert env._policy_cache[id(policy)] == (policy, env._lib._policies[0])
    assert r["obs"].shape == (H, N, env.obs_dim) and ev["record"].shape == (N, EVAL_WORDS) and nav["record"].shape == (N, NAV_WORDS)
    assert int(nav["steps"].max()) == H
    # a handle passed in is used as it is
    handle = env._lib._policies[0]
    env.evaluate_policy(handle, H, out=ev, accumulate=True)
    assert env._lib._policies == [handle] and len(env._policy_cache) == 1
    env.step(torch.zeros((N, env.act_dim), device="cuda:0"))
    env.step_packed(torch.zeros((N, env.act_dim), device="cuda:0"))
    assert env._step_cache is not None and list(env._packed_cache) == [True] and "obs" in env._bufs
    torch.cuda.synchronize()
    lib = env._lib
    env.close()
    assert lib._policies == [] and not handle._p and not lib._h
    assert env._policy_cache == {} and env._step_cache is None and env._packed_cache == {} and env._bufs == {}


@pytest.mark.parametrize("call, words", [("evaluate_policy", EVAL_WORDS), ("evaluate_navigation", NAV_WORDS)])
def test_evaluations_refuse_a_block_they_cannot_write(call, words):
    import torch
    policy = pursuit_mlp(3.0)
    dev, hst = snake("torch"), snake("numpy")

    def run(env, out):
        if call == "evaluate_policy":
            return env.evaluate_policy(policy, H, out=out)
        return env.evaluate_navigation(policy, H, LINE, out=out)

    shape = rf"^out must be an int32 \[{N}, {words}\] block$"
    with pytest.raises(ValueError, match=shape):
        run(dev, torch.zeros((N, words - 1), dtype=torch.int32, device="cuda:0"))
    with pytest.raises(ValueError, match=shape):
        run(hst, np.zeros((N + 1, words), np.int32))
    with pytest.raises(ValueError, match=r"^out must be a torch tensor on cuda:0$"):
        run(dev, np.zeros((N, words), np.int32))
    with pytest.raises(ValueError, match=r"^out must be a torch tensor on cuda:0$"):
        run(dev, torch.zeros((N, words), dtype=torch.int32))                 # a tensor, but on the host
    with pytest.raises(ValueError, match=r"^out must be a numpy array \(this env returns host arrays\)$"):
        run(hst, torch.zeros((N, words), dtype=torch.int32, device="cuda:0"))
    with pytest.raises(ValueError, match=rf"^record must be a contiguous int32 \[N, {words}\] block$"):
        run(dev, torch.zeros((N, words), dtype=torch.float32, device="cuda:0"))
    # a block of the right kind is taken, and is the one returned
    for env, good in ((dev, torch.zeros((N, words), dtype=torch.int32, device="cuda:0")), (hst, np.zeros((N, words), np.int32))):
        assert run(env, good)["record"] is good
    torch.cuda.synchronize()
    dev.close()
    hst.close()


def mask_forms():
    import torch
    return [MASK.tolist(), MASK.copy(), torch.from_numpy(MASK).to("cuda:0")]


def test_snake_reset_takes_a_mask_in_every_form():
    import torch
    envs = [snake() for _ in range(3)]
    rng = np.random.default_rng(2)
    acts = rng.uniform(-1, 1, (H, N, envs[0].act_dim)).astype(np.float32)
    got = []
    for e, m in zip(envs, mask_forms()):
        first = host(e.reset()[0]).copy()
        for t in range(H):
            e.step(acts[t])
        moved = host(e.observe()).copy()
        obs = host(e.reset(mask=m)[0]).copy()
        assert not np.array_equal(moved[MASK], first[MASK]) and np.array_equal(obs[~MASK], moved[~MASK])
        assert not np.array_equal(obs[MASK], moved[MASK])
        got.append((obs, host(e.observe()).copy()))
    torch.cuda.synchronize()
    for k in (1, 2):
        assert same(got[0][0], got[k][0]) and same(got[0][1], got[k][1]), k
    assert same(got[0][0], got[0][1])
    for e in envs:
        e.close()


def test_robot_reset_takes_a_mask_in_every_form():
    import torch
    envs = [SalpRobotVectorEnv(N, device="cuda:0", seed=SEED) for _ in range(3)]
    acts = np.random.default_rng(3).uniform(0, 1, (N, 3)).astype(np.float32) * np.array([1.0, 0.05, 1.0], np.float32)
    got = []
    for e, m in zip(envs, mask_forms()):
        e.reset()
        e.step(acts)
        moved = host(e.observe()).copy()
        obs = host(e.reset(mask=m)[0]).copy()
        assert np.array_equal(obs[~MASK], moved[~MASK]) and not np.array_equal(obs[MASK], moved[MASK])
        got.append((obs, host(e.observe()).copy(), e.get_state()))
    torch.cuda.synchronize()
    for k in (1, 2):
        assert all(same(a, b) for a, b in zip(got[0], got[k])), k
    assert same(got[0][0], got[0][1])
    for e in envs:
        e.close()
    # the numpy env takes the same forms on the host
    hosts = [SalpRobotVectorEnv(N, device="cuda:0", seed=SEED, output="numpy") for _ in range(2)]
    for e, m in zip(hosts, (MASK.tolist(), MASK.astype(np.float64))):
        e.reset()
        e.step(acts)
        assert same(e.reset(mask=m)[0], got[0][0])
    for e in hosts:
        e.close()
