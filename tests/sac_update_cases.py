"""The cases of the SAC update tests and the one comparison they share (tests/test_sac_update.py on the CPU,
tests/test_gpu_sac_update.py on the device, eager and captured): a learner put into a state where every term of the update
matters, the test's own noise in place of `torch.randn_like`, and `check_update`, which runs ONE update of the learner and
judges every observable quantity of it against tests/sac_reference.py.

Each update is judged on its own: the restatement is loaded from the learner's state (float32, cast to float64) before
the update, the critic of the actor stage is the learner's own stepped critic, and the restated Adam / polyak steps are
fed the learner's own float32 gradients (with float64 moments kept by the restatement across updates), so an optimiser's
amplification of a last-bit difference is not carried from one check to the next.

Allowance: the restatement is run in float64 and in float32; with d their difference relative to the quantity's max-abs,
the learner must be within max(16 d, 2^-20) of the float64 run (16: the learner's GEMMs and reductions sum in another
order).  What is compared with a restated Adam or polyak step starts from the learner's own float32 inputs: 2^-20."""
import torch
import torch.nn as nn

import sac_reference as R
from underwater_swimmer_rl_amd.sac import SAC, SACConfig

OBS_DIM = 24
FLOOR = 2.0 ** -20
FACTOR = 16.0
NOISE_SCALE = 0.15          # eps = 0.15 * clip(randn, -3, 3): |eps| <= 0.45 (sac_reference.py says why)
F64, F32 = torch.float64, torch.float32

CASES = {
    # sac_gail.yaml's agent block on a small net
    "h32_fixed_alpha": dict(hidden=(32, 32), batch=128, low=[-1.0], high=[1.0], alpha=0.1, learn_alpha=False, lr=3e-4,
                            alpha_lr=3e-4, gamma=0.99, tau=0.005, target_entropy=-1.0, seed=11),
    # every hyper-parameter off its default, and large enough steps that the order of critic step, actor loss and polyak shows
    "h64_learned_alpha": dict(hidden=(64, 64), batch=256, low=[0.0, -1.0], high=[1.0, 1.0], alpha=0.3, learn_alpha=True,
                              lr=3e-3, alpha_lr=1e-3, gamma=0.97, tau=0.1, target_entropy=-1.5, seed=12),
    # SB3's defaults: alpha learned from 1, target entropy -|A|
    "h256_learned_alpha": dict(hidden=(256, 256), batch=128, low=[0.0, -1.0], high=[1.0, 1.0], alpha=None, learn_alpha=True,
                               lr=3e-4, alpha_lr=3e-4, gamma=0.995, tau=0.005, target_entropy=None, seed=13),
}


def hyper(case):
    c = CASES[case]
    te = -float(len(c["low"])) if c["target_entropy"] is None else c["target_entropy"]
    return dict(gamma=c["gamma"], tau=c["tau"], lr=c["lr"], alpha_lr=c["alpha_lr"], target_entropy=te, learn_alpha=c["learn_alpha"])


def make_agent(case, device="cpu"):
    """The learner of a case: critic_target perturbed away from critic, and the bias of the log-std head's unit 0 raised to
    the clamp, so that the clamp at 2 is active on about half of the rows (unit 1, where there is one, stays below it);
    `check_update` re-centres it on each batch (`centre_clamp`)."""
    c = CASES[case]
    cfg = SACConfig(hidden_sizes=c["hidden"], learning_rate=c["lr"], batch_size=c["batch"], gamma=c["gamma"], tau=c["tau"],
                    alpha=c["alpha"], target_entropy=c["target_entropy"], alpha_lr=c["alpha_lr"])
    agent = SAC(OBS_DIM, len(c["low"]), cfg, device=device, act_low=c["low"], act_high=c["high"], learn_alpha=c["learn_alpha"],
                seed=c["seed"])
    g = torch.Generator().manual_seed(c["seed"])
    with torch.no_grad():
        for p in agent.critic_target.parameters():
            p.add_((0.05 * torch.randn(p.shape, generator=g)).to(p.device))
        agent.actor.log_std.bias[0] = R.LOG_STD_MAX
    return agent


@torch.no_grad()
def centre_clamp(agent, batch):
    """Moves the raised bias so that the clamp lies half-way between the two middle values of unit 0's log-std, before the
    clamp, over the batch's rows (obs and next_obs): half of the rows on either side and none AT the clamp, where float32 and
    float64 would disagree about the side.  The updates themselves carry it away from there, by lr per step and more through
    the body."""
    raw = agent.actor.log_std(agent.actor.body(torch.cat([batch[0], batch[3]])))[:, 0].sort().values
    k = raw.numel() // 2
    agent.actor.log_std.bias[0] += R.LOG_STD_MAX - 0.5 * (raw[k - 1] + raw[k])


def make_batch(case, k, device="cpu", all_terminated=False):
    """Batch k of a case (about 30 % terminated rows) and its two noise tensors (next-state action, policy action)."""
    c = CASES[case]
    g = torch.Generator().manual_seed(1000 * c["seed"] + k)
    B, low, high = c["batch"], torch.tensor(c["low"]), torch.tensor(c["high"])
    r = lambda *s: torch.randn(*s, generator=g)
    obs, next_obs, rew = r(B, OBS_DIM), r(B, OBS_DIM), r(B)
    act = low + (high - low) * torch.rand(B, len(low), generator=g)
    term = torch.ones(B) if all_terminated else (torch.rand(B, generator=g) < 0.3).float()
    eps = [NOISE_SCALE * r(B, len(low)).clamp(-3, 3) for _ in range(2)]
    return tuple(t.to(device) for t in (obs, act, rew, next_obs, term)), [e.to(device) for e in eps]


class Noise:
    """What the tests put in place of `torch.randn_like`: two static tensors handed out in turn (the first draw of an update
    belongs to the next-state action, the second to the policy action), refilled in place with `fill`."""

    def __init__(self, case, device="cpu"):
        c = CASES[case]
        self.t = [torch.zeros(c["batch"], len(c["low"]), device=device) for _ in range(2)]
        self.calls = 0

    def fill(self, eps):
        for t, e in zip(self.t, eps):
            t.copy_(e)

    def __call__(self, like, **kw):
        t = self.t[self.calls % 2]
        assert t.shape == like.shape and t.device == like.device and not kw
        self.calls += 1
        return t


def _linears(seq):
    return [(m.weight, m.bias) for m in seq if isinstance(m, nn.Linear)]


def export(agent, case):
    """The learner's state as the restatement's dict, float64 on the CPU."""
    a, c = agent.actor, CASES[case]
    s = {"actor": {"body": _linears(a.body), "mu": (a.mu.weight, a.mu.bias), "log_std": (a.log_std.weight, a.log_std.bias)},
         "q1": _linears(agent.critic.q1), "q2": _linears(agent.critic.q2), "q1_target": _linears(agent.critic_target.q1),
         "q2_target": _linears(agent.critic_target.q2), "log_alpha": agent.log_alpha,
         "low": torch.tensor(c["low"]), "high": torch.tensor(c["high"])}
    return R.cast(s, F64)


def moments_for(state):
    return {"critic": R.adam_moments(R.critic_flat(state)), "actor": R.adam_moments(R.actor_flat(state["actor"])),
            "log_alpha": R.adam_moments([state["log_alpha"]])}


def rel_diff(x, ref):
    """max |x - ref| relative to max |ref| (0 where both are all zero)."""
    x, ref = torch.as_tensor(x).detach().cpu().to(F64), torch.as_tensor(ref).detach().cpu().to(F64)
    assert x.shape == ref.shape and torch.isfinite(ref).all()
    scale = float(ref.abs().max())
    if scale == 0.0:
        return 0.0 if float(x.abs().max()) == 0.0 else float("inf")
    return float((x - ref).abs().max()) / scale


def allowance(ref64, ref32):
    d = rel_diff(ref32, ref64)
    return max(FACTOR * d, FLOOR), d


class Worst:
    """The largest learner / allowance ratio and the largest float32-vs-float64 figure per kind of quantity."""

    def __init__(self):
        self.ratio, self.d = {}, {}

    def judge(self, kind, label, got, ref64, ref32=None):
        allow, d = (FLOOR, None) if ref32 is None else allowance(ref64, ref32)
        ratio = rel_diff(got, ref64) / allow
        self.ratio[kind] = max(self.ratio.get(kind, 0.0), ratio)
        if d is not None:
            self.d[kind] = max(self.d.get(kind, 0.0), d)
        assert ratio <= 1.0, f"{label}: {kind} is {ratio:.3g} x its allowance {allow:.3g} (relative to max-abs)"

    def line(self, case):
        r = ", ".join(f"{k} {v:.2g}" for k, v in self.ratio.items())
        d = ", ".join(f"{k} {v:.2g}" for k, v in self.d.items())
        return f"{case}: worst learner / allowance: {r}; float32 vs float64 restatement: {d}"


def run_stages(agent, batch):
    """One eager update, stage by stage as `SAC.update` runs them: what `check_update` needs to see of it."""
    def run():
        agent.stage_critic(batch)
        if agent.exchange:
            agent._all_reduce_mean(agent._flat_c)
        grads = [p.grad.detach().clone() for p in agent.critic.parameters()]
        agent.stage_actor()
        if agent.exchange:
            agent._all_reduce_mean(agent._flat_a)
        metrics = agent.stage_finish()
        agent.updates += 1
        return grads, metrics
    return run


def check_update(case, agent, batch, eps, moments, run, worst, label):
    """One update of the learner, `run() -> (the critic's gradients after stage_critic, the returned metrics)`, against the
    restatement.  `moments`: the restated optimisers' float64 moments (`moments_for`), advanced here."""
    hp = hyper(case)
    centre_clamp(agent, batch)
    before = export(agent, case)
    b64, e64 = R.cast(batch, F64), R.cast(eps, F64)
    b32, e32, before32 = R.cast(batch, F32), R.cast(eps, F32), R.cast(before, F32)
    critic_grad, metrics = run()
    after = export(agent, case)
    J = lambda kind, *a: worst.judge(kind, f"{case} {label}", *a)

    # stage_critic: the loss and every gradient
    c, c32 = R.critic_stage(before, b64, e64[0], hp), R.critic_stage(before32, b32, e32[0], hp)
    J("critic_loss", metrics["critic_loss"], c["critic_loss"], c32["critic_loss"])
    assert len(critic_grad) == len(c["critic_grad"])
    for g, r64, r32 in zip(critic_grad, c["critic_grad"], c32["critic_grad"]):
        J("critic_grad", g, r64, r32)
    # stage_actor: the critic's step on the learner's own gradients ...
    stepped, moments["critic"] = R.adam_step(R.critic_flat(before), R.cast(list(critic_grad), F64), moments["critic"], hp["lr"])
    for p, r in zip(R.critic_flat(after), stepped):
        J("critic", p, r)
    # ... and the actor / entropy-coefficient losses on the learner's own stepped critic
    s64 = R.with_critic(before, R.critic_flat(after))
    a, a32 = R.actor_stage(s64, b64[0], e64[1], hp), R.actor_stage(R.cast(s64, F32), b32[0], e32[1], hp)
    J("actor_loss", metrics["actor_loss"], a["actor_loss"], a32["actor_loss"])
    J("entropy", metrics["entropy"], a["entropy"], a32["entropy"])
    actor_grad = [p.grad for p in agent.actor.parameters()]
    for g, r64, r32 in zip(actor_grad, a["actor_grad"], a32["actor_grad"]):
        J("actor_grad", g, r64, r32)
    # stage_finish: the actor's and log_alpha's steps, the polyak update with the stepped critic, the metrics
    stepped, moments["actor"] = R.adam_step(R.actor_flat(before["actor"]), R.cast(actor_grad, F64), moments["actor"], hp["lr"])
    for p, r in zip(R.actor_flat(after["actor"]), stepped):
        J("actor", p, r)
    if hp["learn_alpha"]:
        J("log_alpha_grad", agent.log_alpha.grad, a["log_alpha_grad"], a32["log_alpha_grad"])
        (la,), moments["log_alpha"] = R.adam_step([before["log_alpha"]], [R.cast(agent.log_alpha.grad, F64)], moments["log_alpha"],
                                                  hp["alpha_lr"])
        J("log_alpha", after["log_alpha"], la)
    else:       # fixed alpha: bit-unchanged
        assert agent.log_alpha.grad is None and torch.equal(after["log_alpha"], before["log_alpha"])
    for p, r in zip(R.critic_flat(after, R.TARGETS), R.polyak(R.critic_flat(before, R.TARGETS), R.critic_flat(after), hp["tau"])):
        J("target", p, r)
    J("alpha", metrics["alpha"], after["log_alpha"].exp())
    # both kinds of row: the clamp at LOG_STD_MAX active and inactive
    for stage in (c, a):
        frac = float(stage["clamped"].double().mean())
        assert 0.1 <= frac <= 0.9, f"{case} {label}: clamp active on {frac:.2f} of the rows"
    frac = float(b64[4].mean())
    assert 0.15 <= frac <= 0.45, frac
