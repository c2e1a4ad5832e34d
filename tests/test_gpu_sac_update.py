"""The SAC learner on the device: the update with capturable fused Adam, eager and replayed from captured
graphs, against the CPU float64 restatement (tests/sac_reference.py; cases, comparison and allowance rule:
tests/sac_update_cases.py), and what `train_sac`, `train_sac_graphed` and its segmented form put into the replay buffer,
row for row against a twin env stepped with the buffer's own actions.

Measured on an MI355X, worst over all updates (eager, warm-up and replay) and the tensors of a kind: float32 vs float64
restatement d 4.5e-8 .. 1.1e-7 (losses, entropy, log_alpha gradient), 3.5e-7 .. 5.5e-7 (critic gradients), 1.0e-6 .. 3.0e-6
(actor gradients); learner / allowance at most 0.14 (critic and actor gradients, h64), 0.12 against the restated steps
(target); one graph and three graphs give the same figures as each other.  The snake loops stored 371 terminated and 653
truncated rows of 24576 with 75 mixed (step, wavefront) pairs, the robot loops 91 terminated and 956 truncated of 3072, the
same in all three loops.

The robot run uses the 100 x 100 tank with margin 50: there the CPU oracle, under uniform actions, reaches a target on 90
of the 3072 rows (and truncates 953 by the cycle count, max_cycles = 3), in the default tank on none; the floor on
terminated rows is half of that, 45."""
import pytest
import torch

import sac_update_cases as S
import underwater_swimmer_rl_amd as pkg
from underwater_swimmer_rl_amd.sac import SAC, DeviceReplayBuffer, SACConfig, train_sac, train_sac_graphed

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GPU_CASES = ["h64_learned_alpha", "h256_learned_alpha"]
WARMUP = UPDATES = 3


@pytest.mark.parametrize("case", GPU_CASES)
def test_three_updates_on_the_device(case, monkeypatch):
    agent = S.make_agent(case, DEV)
    noise = S.Noise(case, DEV)
    monkeypatch.setattr(torch, "randn_like", noise)
    moments, worst = S.moments_for(S.export(agent, case)), S.Worst()
    for k in range(UPDATES):
        batch, eps = S.make_batch(case, k, DEV)
        noise.fill(eps)
        S.check_update(case, agent, batch, eps, moments, S.run_stages(agent, batch), worst, f"update {k + 1}")
    assert noise.calls == 2 * UPDATES
    print(worst.line(case + " on the device"))


def _refill(case, k, static_batch, noise):
    batch, eps = S.make_batch(case, k, DEV)
    for dst, src in zip(static_batch, batch):
        dst.copy_(src)
    noise.fill(eps)
    return eps


def _critic_grads_of(agent, flat):
    out, o = [], 0
    for p in agent.critic.parameters():
        out.append(flat[o:o + p.numel()].view_as(p).clone())
        o += p.numel()
    return out


@pytest.mark.parametrize("segments", [False, True], ids=["one_graph", "three_stage_graphs"])
@pytest.mark.parametrize("case", GPU_CASES)
def test_captured_updates_replay_the_new_batch_and_noise(case, segments, monkeypatch):
    """Three eager warm-up updates on a side stream as `train_sac_graphed` runs them, then `agent.update(batch)` captured in
    one graph — or the three stages in three graphs with exchange=True, keep_grads=True — and replayed three times, batch
    and noise refilled in place before each replay: a captured constant, a stale batch or action, or an Adam step count that
    does not advance on replay would be outside the allowance.  Every update, warm-up and replay, is judged.  The critic's
    gradients of the one-graph form are copied out between the stages (stage_actor's backward adds to them)."""
    agent = S.make_agent(case, DEV)
    agent.exchange = segments
    noise = S.Noise(case, DEV)
    monkeypatch.setattr(torch, "randn_like", noise)
    static_batch, _ = S.make_batch(case, 0, DEV)
    critic_params = list(agent.critic.parameters())
    snap = [torch.zeros_like(p) for p in critic_params]
    stage_actor = agent.stage_actor

    def probed_stage_actor():
        torch._foreach_copy_(snap, [p.grad for p in critic_params])
        stage_actor()
    agent.stage_actor = probed_stage_actor
    moments, worst = S.moments_for(S.export(agent, case)), S.Worst()
    side = torch.cuda.Stream(device=DEV)

    def eager():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            metrics = agent.update(static_batch)
        torch.cuda.current_stream().wait_stream(side)
        return [s.clone() for s in snap], metrics
    for k in range(WARMUP):
        eps = _refill(case, k, static_batch, noise)
        S.check_update(case, agent, static_batch, eps, moments, eager, worst, f"warm-up {k + 1}")
    torch.cuda.synchronize()
    graphs, out = [], {}
    if segments:
        agent.keep_grads = True
        pool = torch.cuda.graph_pool_handle()
        for stage in (lambda: agent.stage_critic(static_batch), agent.stage_actor, lambda: out.update(agent.stage_finish())):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool):
                stage()
            graphs.append(g)
    else:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out.update(agent.update(static_batch))
        graphs.append(g)
    before = S.export(agent, case)

    def replay():
        if not segments:
            graphs[0].replay()
            return [s.clone() for s in snap], out
        graphs[0].replay()
        agent._all_reduce_mean(agent._flat_c)
        grads = _critic_grads_of(agent, agent._flat_c)
        graphs[1].replay()
        agent._all_reduce_mean(agent._flat_a)
        graphs[2].replay()
        return grads, out
    for k in range(UPDATES):
        eps = _refill(case, WARMUP + k, static_batch, noise)
        if k == 0:      # capture ran no kernel
            now = S.export(agent, case)
            assert all(torch.equal(a, b) for a, b in zip(S.R.critic_flat(before), S.R.critic_flat(now)))
        S.check_update(case, agent, static_batch, eps, moments, replay, worst, f"replay {k + 1}")
    assert moments["critic"]["t"] == WARMUP + UPDATES
    print(worst.line(f"{case}, {'three graphs' if segments else 'one graph'}"))


# ---------------------------------------------------------------------------------------------- what the training loops store
SNAKE_OVERRIDES = dict(num_food_items=3, width=300, height=300, max_steps_without_food=16, max_thrust_force=400,
                       inhale_duration=4, exhale_duration=20, rest_duration=4)
ROBOT_ORACLE_TERMINATED = 90       # target-reached rows of the CPU oracle in this tank, 256 robots x 12 steps, uniform actions
LOOPS = {"train_sac": (train_sac, {}), "train_sac_graphed": (train_sac_graphed, {}),
         "train_sac_graphed_segments": (train_sac_graphed, {"force_segments": True})}


def _twin_check(make_env, loop, steps, learning_starts):
    """Runs the loop into a buffer that does not wrap, then steps a fresh env of the same seed with the buffer's own action
    rows and compares every block bit for bit.  Returns the twin's flags [steps, n] and the run's metrics."""
    run, kw = LOOPS[loop]
    env = make_env()
    n = env.num_envs
    cfg = SACConfig(hidden_sizes=(32, 32), batch_size=128, learning_starts=learning_starts)
    agent = SAC(env.obs_dim, env.act_dim, cfg, device=DEV, seed=0, act_low=env.single_action_space.low,
                act_high=env.single_action_space.high)
    buffer = DeviceReplayBuffer(steps * n, env.obs_dim, env.act_dim, DEV)
    for t in (buffer.obs, buffer.next_obs, buffer.act, buffer.rew, buffer.term):
        t.fill_(float("nan"))
    m = run(env, agent, steps, buffer=buffer, **kw)
    assert m["vector_steps"] == steps and buffer.size == steps * n and buffer.pos == 0
    assert m["updates"] == steps - learning_starts
    stats = env.stats() if hasattr(env, "stats") else None
    env.close()

    twin = make_env()
    obs, _ = twin.reset()
    obs = obs.clone()
    ep = torch.zeros(n, device=DEV)
    ret, episodes = 0.0, 0
    terms, truncs = [], []
    for t in range(steps):
        sl = slice(t * n, (t + 1) * n)
        assert torch.equal(buffer.obs[sl], obs), f"step {t}: obs is not the twin's current observation"
        nobs, rew, term, trunc, info = twin.step(buffer.act[sl].clone())
        done = term | trunc
        assert torch.equal(buffer.rew[sl], rew), f"step {t}: reward"
        assert torch.equal(buffer.term[sl], term.to(torch.float32)), f"step {t}: term is not `terminated`"
        want = torch.where(done[:, None], info["final_observation"], nobs)
        assert torch.equal(buffer.next_obs[sl], want), f"step {t}: next_obs"
        if done.any():      # the terminal row, not the post-reset one: they differ wherever an episode ended
            assert not torch.equal(want[done], nobs[done])
        ep += rew
        ret += float(ep[done].double().sum())
        episodes += int(done.sum())
        ep[done] = 0.0
        terms.append(term.clone())
        truncs.append(trunc.clone())
        obs = nobs.clone()
    assert m["episodes"] == episodes
    assert abs(m["mean_return"] - ret / max(episodes, 1)) <= 1e-5 * abs(ret / max(episodes, 1))
    if stats is not None:
        assert stats == twin.stats()
    twin.close()
    return torch.stack(terms).cpu().numpy(), torch.stack(truncs).cpu().numpy(), m


@pytest.mark.parametrize("loop", list(LOOPS))
def test_what_the_loops_store_on_the_snake_env(loop):
    steps, n, starts = 48, 512, 24
    make = lambda: pkg.SalpVectorEnv("sac_gail", num_envs=n, device=DEV, seed=5, **SNAKE_OVERRIDES)
    term, trunc, m = _twin_check(make, loop, steps, starts)
    done = (term | trunc).reshape(steps, n // 64, 64)
    mixed = int((done.any(-1) & ~done.all(-1)).sum())
    print(f"{loop}: terminated {int(term.sum())}, truncated {int(trunc.sum())} of {steps * n} rows, mixed (step, wavefront) pairs {mixed}")
    # the CPU oracle under uniform actions gave 388 terminated and 636 truncated rows of 24576 for this config
    assert term.sum() >= 100 and trunc.sum() >= 100 and mixed >= 1
    if loop != "train_sac":
        assert m["segmented"] is (loop == "train_sac_graphed_segments")


@pytest.mark.parametrize("loop", list(LOOPS))
def test_what_the_loops_store_on_the_robot_env(loop):
    steps, n, starts, cycles = 12, 256, 6, 3
    make = lambda: pkg.SalpRobotVectorEnv(n, device=DEV, seed=1, max_cycles=cycles, width=100, height=100, tank_margin=50.0)
    term, trunc, m = _twin_check(make, loop, steps, starts)
    print(f"{loop}: terminated {int(term.sum())}, truncated {int(trunc.sum())} of {steps * n} rows")
    # an episode is at most `cycles` steps long, so every robot ends one in each phase; nearly all of them by truncation
    done = term | trunc
    assert done[:starts].any(0).all() and done[starts:].any(0).all()
    assert trunc[:starts].sum() >= n // 2 and trunc[starts:].sum() >= n // 2
    assert (done.sum(0) >= steps // cycles).all()
    assert term.sum() >= ROBOT_ORACLE_TERMINATED // 2
