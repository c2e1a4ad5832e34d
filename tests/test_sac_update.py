"""What one SAC update IS: `SAC.stage_critic / stage_actor / stage_finish` on the CPU against the float64
restatement of tests/sac_reference.py, three consecutive updates per case (Adam's steps 1, 2, 3 and a target network that
has moved), the test's own noise in place of `torch.randn_like` (tests/sac_update_cases.py has the cases, the comparison
and the allowance rule); a mutant guard that proves the comparison can fail; the three gradient-exchange forms bit for
bit; the capturable replay sampling below capacity.

Measured on the CPU, worst over the three updates and the tensors of a kind:
  float32 vs float64 restatement, d relative to max-abs: critic loss 6.5e-8 .. 8.9e-8, critic gradients 4.0e-7 .. 4.8e-7,
    actor loss 5.5e-8 .. 9.4e-7, actor gradients 6.5e-7 .. 1.1e-6, log_alpha gradient 7e-8, entropy 4.5e-8 .. 1.0e-7
  learner / allowance (the allowance being max(16 d, 2^-20)): h32 0.12 (actor gradients), h64 0.15 (actor loss),
    h256 0.23 (actor gradients); against the restated Adam and polyak steps (2^-20 alone) at most 0.12 (target)
  mutants: the weakest (the polyak update with the pre-step critic) moves a target tensor 4.1e3 x its allowance, the next
    (the target critics seeing tanh(u)) 4.9e4 x, every other one 6e4 x .. 2.3e6 x
On an MI355X (tests/test_gpu_sac_update.py): d as above within a factor of three, learner / allowance at most 0.14."""
import pytest
import torch

import sac_reference as R
import sac_update_cases as S
from underwater_swimmer_rl_amd.sac import DeviceReplayBuffer

UPDATES = 3
MUTANT_FACTOR = 1000.0
STEPPED = ("critic/", "actor/", "target/", "log_alpha", "alpha")     # compared with a restated step: the floor alone


@pytest.mark.parametrize("case", list(S.CASES))
def test_three_updates_against_the_restatement(case, monkeypatch):
    agent = S.make_agent(case)
    noise = S.Noise(case)
    monkeypatch.setattr(torch, "randn_like", noise)
    moments, worst = S.moments_for(S.export(agent, case)), S.Worst()
    for k in range(UPDATES):
        batch, eps = S.make_batch(case, k)
        noise.fill(eps)
        S.check_update(case, agent, batch, eps, moments, S.run_stages(agent, batch), worst, f"update {k + 1}")
    assert noise.calls == 2 * UPDATES and agent.updates == UPDATES and moments["critic"]["t"] == UPDATES
    print(worst.line(case))


@pytest.mark.parametrize("case", list(S.CASES))
def test_a_terminated_row_has_its_reward_for_target(case, monkeypatch):
    """Through the critic loss of a batch whose rows are all terminated, against the direct formula."""
    agent = S.make_agent(case)
    noise = S.Noise(case)
    monkeypatch.setattr(torch, "randn_like", noise)
    batch, eps = S.make_batch(case, 7, all_terminated=True)
    noise.fill(eps)
    S.centre_clamp(agent, batch)
    agent.stage_critic(batch)
    state = S.export(agent, case)

    def direct(dtype):
        s, (obs, act, rew, _, _) = R.cast(state, dtype), R.cast(batch, dtype)
        q1, q2 = R.twin_q(s["q1"], s["q2"], obs, act)
        return 0.5 * (((q1 - rew) ** 2).mean() + ((q2 - rew) ** 2).mean())
    worst = S.Worst()
    worst.judge("critic_loss", case, agent._carry["critic_loss"], direct(S.F64), direct(S.F32))
    # and the bootstrap is not small here: the same rows, not terminated, give another loss altogether
    open_rows = R.critic_stage(state, R.cast(batch[:4], S.F64) + (torch.zeros(len(batch[4]), dtype=S.F64),), R.cast(eps[0], S.F64),
                               S.hyper(case))
    assert S.rel_diff(open_rows["critic_loss"], direct(S.F64)) > 1e-2


def _restated_update(case, dtype, mutant=None):
    state = S.export(S.make_agent(case), case)
    batch, eps = S.make_batch(case, 0)
    s, b, e = R.cast(state, dtype), R.cast(batch, dtype), R.cast(eps, dtype)
    return R.update(s, S.moments_for(s), b, e[0], e[1], S.hyper(case), mutant)[2]


def test_every_mutant_of_the_restatement_shows():
    """On the restatement alone, at the (64, 64) case: each single mis-statement moves at least one compared quantity by at
    least 1000 x that quantity's allowance."""
    case = "h64_learned_alpha"
    q64, q32 = _restated_update(case, S.F64), _restated_update(case, S.F32)
    allow = {k: S.FLOOR if k.startswith(STEPPED) else S.allowance(q64[k], q32[k])[0] for k in q64}
    assert {"critic_loss", "actor_loss", "entropy", "log_alpha_grad", "log_alpha", "alpha", "critic_grad/0", "actor_grad/0", "critic/0",
            "actor/0", "target/0"} <= set(allow)
    weakest = {}
    for mutant in R.MUTANTS:
        qm = _restated_update(case, S.F64, mutant)
        moved = {k: S.rel_diff(qm[k], q64[k]) / allow[k] for k in q64}
        best = max(moved, key=moved.get)
        weakest[mutant] = (best, moved[best])
        print(f"{mutant}: {best} moves {moved[best]:.3g} x its allowance {allow[best]:.3g}")
    assert len(R.MUTANTS) >= 15
    short = {m: v for m, v in weakest.items() if not v[1] >= MUTANT_FACTOR}
    assert not short, short


def _run_form(case, monkeypatch, exchange, keep_grads):
    agent = S.make_agent(case)
    agent.exchange, agent.keep_grads = exchange, keep_grads
    noise = S.Noise(case)
    monkeypatch.setattr(torch, "randn_like", noise)
    addresses = []
    for k in range(UPDATES):
        batch, eps = S.make_batch(case, k)
        noise.fill(eps)
        agent.update(batch)
        params = [*agent.critic.parameters(), *agent.actor.parameters()] + ([agent.log_alpha] if agent.learn_alpha else [])
        addresses.append([p.grad.data_ptr() for p in params])
    tensors = [*agent.actor.parameters(), *agent.critic.parameters(), *agent.critic_target.parameters(), agent.log_alpha]
    return [t.detach().clone() for t in tensors], addresses


@pytest.mark.parametrize("case", ["h32_fixed_alpha", "h64_learned_alpha"])
def test_the_exchange_forms_leave_the_same_bits(case, monkeypatch):
    plain, _ = _run_form(case, monkeypatch, False, False)
    flat, _ = _run_form(case, monkeypatch, True, False)
    kept, addresses = _run_form(case, monkeypatch, True, True)
    for name, other in (("exchange", flat), ("exchange + keep_grads", kept)):
        assert len(plain) == len(other)
        for i, (a, b) in enumerate(zip(plain, other)):
            assert torch.equal(a, b), f"{name}: tensor {i} differs"
    assert addresses[0] == addresses[1] == addresses[2] and len(set(addresses[0])) == len(addresses[0])


@pytest.mark.parametrize("capacity,rows", [(10, 1), (10, 4), (64, 63), (1000, 7)])
def test_capturable_sampling_stays_below_size(capacity, rows):
    """Storage full of NaN, `rows` < capacity of it written: no sampled row is one of the unwritten ones."""
    buf = DeviceReplayBuffer(capacity, 3, 1, "cpu")
    for t in (buf.obs, buf.next_obs, buf.act, buf.rew, buf.term):
        t.fill_(float("nan"))
    g = torch.Generator().manual_seed(capacity + rows)
    buf.add_capturable(torch.randn(rows, 3, generator=g), torch.randn(rows, 1, generator=g), torch.randn(rows, generator=g),
                       torch.randn(rows, 3, generator=g), torch.rand(rows, generator=g) > 0.5)
    buf.advance_host(rows)
    assert buf.size == rows < capacity and int(buf.size_t) == rows
    torch.manual_seed(0)
    hit = torch.zeros(rows, dtype=torch.bool)
    for _ in range(20):
        sample = buf.sample_capturable(512)
        assert not any(torch.isnan(t).any() for t in sample)
        hit |= (sample[0][:, None, :] == buf.obs[None, :rows, :]).all(-1).any(0)
    assert hit.all()        # and every written row is reachable, the last one included
