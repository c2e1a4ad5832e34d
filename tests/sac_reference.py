"""One SAC update, restated: plain functions on explicit tensors, in the dtype of their inputs (the tests
run them in float64 and, for the allowance, in float32), with autograd for the gradients.  Nothing here comes from
`underwater_swimmer_rl_amd.sac`; it states what stable-baselines3's SAC computes:

  actor    ReLU body, `mu` and `log_std` heads, log_std clamped to [-20, 2];  u = mu + exp(log_std) * eps;
           a = tanh(u) * scale + shift for the Box (low, high);
           logp = sum log N(u; mu, std) - sum log(1 - tanh(u)^2)      (the direct formula; no log(scale) term)
  critic   target = r + gamma * (1 - term) * (min(Q1', Q2')(s', a') - alpha * logp'),  Q' the TARGET networks, a' the
           scaled action, nothing of it differentiated;  loss = 0.5 * (mse(Q1, target) + mse(Q2, target))
  actor    loss = mean(alpha * logp - min(Q1, Q2)(s, a_pi)) with the critic AFTER its optimiser step and alpha detached;
           only the actor's parameters are stepped with it
  alpha    alpha_loss = -log_alpha * mean(logp + target_entropy); absent when alpha is fixed (log_alpha then stays)
  Adam     the textbook step with bias correction, beta (0.9, 0.999), eps 1e-8, on a gradient handed to it
  polyak   target <- (1 - tau) * target + tau * critic, after the actor step, with the stepped critic
  noise    the first draw of an update belongs to the next-state action, the second to the policy action

A state is a dict: "actor" = {"body": [(W, b), ...], "mu": (W, b), "log_std": (W, b)}, "q1" / "q2" / "q1_target" /
"q2_target" = [(W, b), ...], "log_alpha" = 0-dim tensor, "low" / "high" = the Box.  `hp` is a dict of Python numbers:
gamma, tau, lr, alpha_lr, target_entropy, learn_alpha.

The direct log(1 - tanh(u)^2) loses all its digits once tanh(u) rounds to 1 (|u| > 8.7 in float32, 18.7 in float64) and
half of them long before, so the tests keep |u| below about 5: their noise is bounded by 0.45, well inside the |eps| <= 3
that the formula needs at std = 1, because the clamped rows have std = e^2.

`MUTANTS`: single mis-statements of the above, each a keyword that switches one line below (tests/test_sac_update.py
proves that each would be seen)."""
import math

import torch

LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8

MUTANTS = {
    "target_without_one_minus_term": "the target bootstraps through terminated rows",
    "target_from_critic": "the target bootstraps from the critic, not from critic_target",
    "target_entropy_sign": "+ alpha * logp' in the target",
    "actor_entropy_sign": "- alpha * logp in the actor loss",
    "target_mean_for_min": "mean of the twin target critics",
    "actor_mean_for_min": "mean of the twin critics in the actor loss",
    "alpha_not_detached": "log_alpha receives the actor loss's gradient",
    "actor_sees_prestep_critic": "the actor loss uses the critic from before its optimiser step",
    "tau_swapped": "target <- tau * target + (1 - tau) * critic",
    "polyak_prestep_critic": "the polyak update uses the critic from before its optimiser step",
    "alpha_loss_sign": "alpha_loss = +log_alpha * mean(logp + target_entropy)",
    "target_entropy_dropped": "alpha_loss = -log_alpha * mean(logp)",
    "no_tanh_correction": "logp without - sum log(1 - tanh(u)^2)",
    "target_unscaled_action": "the target critics see tanh(u), not the Box action",
    "adam_without_bias_correction": "Adam steps with m and v as they are",
}

NETS = ("q1", "q2")
TARGETS = ("q1_target", "q2_target")


# ------------------------------------------------------------------ states as flat lists
def layers_flat(layers):
    return [t for Wb in layers for t in Wb]


def layers_like(layers, flat):
    it = iter(flat)
    return [(next(it), next(it)) for _ in layers]


def actor_flat(actor):
    """The actor's tensors in the order body, mu, log_std (the order of the learner's `actor.parameters()`)."""
    return layers_flat(actor["body"]) + list(actor["mu"]) + list(actor["log_std"])


def actor_like(actor, flat):
    n = 2 * len(actor["body"])
    return {"body": layers_like(actor["body"], flat[:n]), "mu": tuple(flat[n:n + 2]), "log_std": tuple(flat[n + 2:n + 4])}


def critic_flat(state, names=NETS):
    return layers_flat(state[names[0]]) + layers_flat(state[names[1]])


def with_critic(state, flat, names=NETS):
    n = 2 * len(state[names[0]])
    return {**state, names[0]: layers_like(state[names[0]], flat[:n]), names[1]: layers_like(state[names[1]], flat[n:])}


def cast(x, dtype):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device="cpu", dtype=dtype) if x.is_floating_point() else x.detach().cpu()
    if isinstance(x, dict):
        return {k: cast(v, dtype) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(cast(v, dtype) for v in x)
    return x


def _leaves(flat):
    return [t.detach().clone().requires_grad_(True) for t in flat]


# ------------------------------------------------------------------ the networks
def mlp(layers, x):
    for W, b in layers[:-1]:
        x = torch.relu(x @ W.T + b)
    W, b = layers[-1]
    return x @ W.T + b


def twin_q(q1, q2, obs, act):
    x = torch.cat([obs, act], dim=-1)
    return mlp(q1, x).squeeze(-1), mlp(q2, x).squeeze(-1)


def actor_sample(actor, low, high, obs, eps, mutant=None):
    """(Box action, tanh(u), logp, rows on which the clamp at LOG_STD_MAX is active)."""
    h = obs
    for W, b in actor["body"]:
        h = torch.relu(h @ W.T + b)
    mu = h @ actor["mu"][0].T + actor["mu"][1]
    raw = h @ actor["log_std"][0].T + actor["log_std"][1]
    log_std = raw.clamp(LOG_STD_MIN, LOG_STD_MAX)
    std = log_std.exp()
    u = mu + std * eps
    t = torch.tanh(u)
    scale, shift = (high - low) / 2, (high + low) / 2
    logp = (-0.5 * ((u - mu) / std) ** 2 - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
    if mutant != "no_tanh_correction":
        logp = logp - torch.log(1 - t ** 2).sum(-1)
    return t * scale + shift, t, logp, (raw.detach() > LOG_STD_MAX).any(-1)


# ------------------------------------------------------------------ the three stages
def critic_stage(state, batch, eps_next, hp, mutant=None):
    """{"critic_loss", "critic_grad": per tensor of critic_flat(state), "target", "clamped"}."""
    obs, act, rew, next_obs, term = batch
    with torch.no_grad():
        alpha = state["log_alpha"].exp()
        a2, t2, logp2, clamped = actor_sample(state["actor"], state["low"], state["high"], next_obs, eps_next, mutant)
        boot = NETS if mutant == "target_from_critic" else TARGETS
        tq1, tq2 = twin_q(state[boot[0]], state[boot[1]], next_obs, t2 if mutant == "target_unscaled_action" else a2)
        v = 0.5 * (tq1 + tq2) if mutant == "target_mean_for_min" else torch.min(tq1, tq2)
        v = v + alpha * logp2 if mutant == "target_entropy_sign" else v - alpha * logp2
        keep = torch.ones_like(term) if mutant == "target_without_one_minus_term" else 1.0 - term
        target = rew + hp["gamma"] * keep * v
    leaves = _leaves(critic_flat(state))
    s = with_critic(state, leaves)
    q1, q2 = twin_q(s["q1"], s["q2"], obs, act)
    loss = 0.5 * (((q1 - target) ** 2).mean() + ((q2 - target) ** 2).mean())
    grads = torch.autograd.grad(loss, leaves)
    return {"critic_loss": loss.detach(), "critic_grad": list(grads), "target": target, "clamped": clamped}


def actor_stage(state, obs, eps_pi, hp, mutant=None, critic_before=None):
    """`state` holds the critic AFTER its step.  {"actor_loss", "actor_grad": per tensor of actor_flat, "log_alpha_grad"
    (None when alpha is fixed), "entropy", "clamped"}."""
    leaves = _leaves(actor_flat(state["actor"]))
    log_alpha = state["log_alpha"].detach().clone().requires_grad_(True)
    alpha = log_alpha.exp() if mutant == "alpha_not_detached" else log_alpha.exp().detach()
    a, _, logp, clamped = actor_sample(actor_like(state["actor"], leaves), state["low"], state["high"], obs, eps_pi, mutant)
    seen = critic_before if mutant == "actor_sees_prestep_critic" else state
    q1, q2 = twin_q(seen["q1"], seen["q2"], obs, a)
    q = 0.5 * (q1 + q2) if mutant == "actor_mean_for_min" else torch.min(q1, q2)
    loss = (-alpha * logp - q).mean() if mutant == "actor_entropy_sign" else (alpha * logp - q).mean()
    out = {"actor_loss": loss.detach(), "entropy": -logp.detach().mean(), "clamped": clamped, "log_alpha_grad": None}
    if hp["learn_alpha"]:
        te = 0.0 if mutant == "target_entropy_dropped" else hp["target_entropy"]
        alpha_loss = -(log_alpha * (logp.detach() + te).mean())
        if mutant == "alpha_loss_sign":
            alpha_loss = -alpha_loss
        total = loss + alpha_loss        # log_alpha is in `loss` only where the mutant leaves alpha attached
        *grads, out["log_alpha_grad"] = torch.autograd.grad(total, leaves + [log_alpha])
    else:
        grads = torch.autograd.grad(loss, leaves)
    out["actor_grad"] = list(grads)
    return out


def adam_moments(params):
    return {"m": [torch.zeros_like(p) for p in params], "v": [torch.zeros_like(p) for p in params], "t": 0}


def adam_step(params, grads, moments, lr, mutant=None):
    """(the stepped parameters, the new moments); `moments` from `adam_moments` or an earlier step."""
    t = moments["t"] + 1
    m = [BETA1 * m0 + (1 - BETA1) * g for m0, g in zip(moments["m"], grads)]
    v = [BETA2 * v0 + (1 - BETA2) * g * g for v0, g in zip(moments["v"], grads)]
    c1, c2 = (1.0, 1.0) if mutant == "adam_without_bias_correction" else (1 - BETA1 ** t, 1 - BETA2 ** t)
    new = [p - lr * (mi / c1) / ((vi / c2).sqrt() + ADAM_EPS) for p, mi, vi in zip(params, m, v)]
    return new, {"m": m, "v": v, "t": t}


def polyak(target, critic, tau, mutant=None):
    keep, take = (tau, 1 - tau) if mutant == "tau_swapped" else (1 - tau, tau)
    return [keep * t + take * c for t, c in zip(target, critic)]


# ------------------------------------------------------------------ a whole update, on the restatement's own gradients
def update(state, moments, batch, eps_next, eps_pi, hp, mutant=None):
    """(new state, new moments, every compared quantity by name).  `moments` = {"critic", "actor", "log_alpha"}."""
    c = critic_stage(state, batch, eps_next, hp, mutant)
    critic_new, mc = adam_step(critic_flat(state), c["critic_grad"], moments["critic"], hp["lr"], mutant)
    stepped = with_critic(state, critic_new)
    a = actor_stage(stepped, batch[0], eps_pi, hp, mutant, critic_before=state)
    actor_new, ma = adam_step(actor_flat(state["actor"]), a["actor_grad"], moments["actor"], hp["lr"], mutant)
    log_alpha, ml = state["log_alpha"], moments["log_alpha"]
    if hp["learn_alpha"]:
        (log_alpha,), ml = adam_step([state["log_alpha"]], [a["log_alpha_grad"]], ml, hp["alpha_lr"], mutant)
    source = state if mutant == "polyak_prestep_critic" else stepped
    target_new = polyak(critic_flat(state, TARGETS), critic_flat(source), hp["tau"], mutant)
    new = with_critic({**stepped, "actor": actor_like(state["actor"], actor_new), "log_alpha": log_alpha}, target_new, TARGETS)
    q = {"critic_loss": c["critic_loss"], "actor_loss": a["actor_loss"], "entropy": a["entropy"], "alpha": log_alpha.exp(),
         "log_alpha": log_alpha}
    if hp["learn_alpha"]:
        q["log_alpha_grad"] = a["log_alpha_grad"]
    for name, tensors in (("critic_grad", c["critic_grad"]), ("critic", critic_new), ("actor_grad", a["actor_grad"]),
                          ("actor", actor_new), ("target", target_new)):
        q.update({f"{name}/{i}": t for i, t in enumerate(tensors)})
    return new, {"critic": mc, "actor": ma, "log_alpha": ml}, q
