"""`policy.MLPPolicy` on the CPU: the public weight layout against a torch `sac.Actor`, the float64 reference against the
actor's own forward pass, argument validation, the forward-error bound, and the recipe guard of the GPU closed-loop cases
(tests/policy_cases.py): on the oracle alone each case must end episodes and drive its actions over most of their range,
with an error bound small enough that the GPU comparison means something."""
import numpy as np
import pytest

import oracle_lib as ol
import parity_cases as pc
import policy_cases as cases
from underwater_swimmer_rl_amd.policy import MLPPolicy, U, pursuit_policy


def _actor(hidden, act_dim=1, free=False, seed=0):
    import torch
    from underwater_swimmer_rl_amd.sac import Actor
    torch.manual_seed(seed)
    low, high = ([0.0, -1.0], [1.0, 1.0]) if free else (None, None)
    return Actor(24, act_dim, hidden=hidden, act_low=low, act_high=high)


@pytest.mark.parametrize("hidden,act_dim,free", [((32, 32), 1, False), ((64, 16), 2, True), ((48,), 1, False), ((16, 64), 1, False),
                                                 ((48, 32), 2, True)])
def test_pack_reproduces_the_actors_parameters(hidden, act_dim, free):
    actor = _actor(hidden, act_dim, free)
    p = MLPPolicy.from_actor(actor)
    w = p.pack()
    assert w.dtype == np.float32 and w.shape == (1, p.words)
    assert (p.hidden, p.obs_dim, p.act_dim, p.out, p.n_policies) == (hidden, 24, act_dim, "tanh", 1)
    import torch.nn as nn
    lin = [m for m in actor.body if isinstance(m, nn.Linear)] + [actor.mu]
    off = 0
    for m in lin:       # nn.Linear's layout: W[out][in] row-major, then b[out]
        W, b = m.weight.detach().numpy(), m.bias.detach().numpy()
        assert np.array_equal(w[0, off:off + W.size].reshape(W.shape), W)
        off += W.size
        assert np.array_equal(w[0, off:off + b.size], b)
        off += b.size
    assert np.array_equal(w[0, off:off + act_dim], actor.scale.numpy())
    assert np.array_equal(w[0, off + act_dim:], actor.shift.numpy())
    assert off + 2 * act_dim == p.words == sum(m.weight.numel() + m.bias.numel() for m in lin) + 2 * act_dim


@pytest.mark.parametrize("hidden,act_dim,free", [((32, 32), 1, False), ((64, 16), 2, True), ((48,), 1, False)])
def test_reference_is_the_actors_deterministic_forward_in_float64(hidden, act_dim, free):
    import torch
    actor = _actor(hidden, act_dim, free, seed=3)
    p = MLPPolicy.from_actor(actor)
    obs = np.random.default_rng(0).uniform(-1.5, 1.5, (5, 37, 24)).astype(np.float32)
    with torch.no_grad():
        want, _ = actor.double()(torch.from_numpy(obs).double(), deterministic=True, with_logprob=False)
    got = p.reference(obs)
    assert got.dtype == np.float64 and got.shape == (5, 37, act_dim)
    assert np.abs(got - want.numpy()).max() <= 1e-14
    if free:
        assert got[..., 0].min() >= 0.0 and got[..., 0].max() <= 1.0


def test_stack_assigns_env_blocks_to_policies():
    ps = [cases.random_policy(24, 1, (16,), "tanh", s, 1.0, 2.0) for s in range(4)]
    pop = MLPPolicy.stack(ps)
    assert pop.n_policies == 4 and pop.pack().shape == (4, ps[0].words)
    assert np.array_equal(pop.pack()[2], ps[2].pack()[0])
    obs = np.random.default_rng(1).uniform(-1, 1, (3, 256, 24)).astype(np.float32)
    got = pop.reference(obs)
    for k, p in enumerate(ps):       # env i runs policy i // (n / P)
        assert np.array_equal(got[:, 64 * k:64 * (k + 1)], p.reference(obs[:, 64 * k:64 * (k + 1)]))
        assert np.array_equal(pop.error_bound(obs)[:, 64 * k:64 * (k + 1)], p.error_bound(obs[:, 64 * k:64 * (k + 1)]))


def test_linear_clip_expresses_the_pursuit_rule():
    p = pursuit_policy(3.0)
    assert p.hidden == () and p.out == "clip" and p.words == 24 + 1 + 2
    obs = np.random.default_rng(2).uniform(-1, 1, (100, 24)).astype(np.float32)
    assert np.array_equal(p.reference(obs)[:, 0], np.clip(-3.0 * obs[:, 13].astype(np.float64), -1.0, 1.0))


def test_argument_validation():
    W = np.zeros((1, 24), np.float32)
    with pytest.raises(ValueError):
        MLPPolicy.linear(W, out="softmax")
    for bad in (8, 24, 80):                                  # not a multiple of 16 in [16, 64]
        with pytest.raises(ValueError):
            MLPPolicy.from_layers([(np.zeros((bad, 24)), np.zeros(bad)), (np.zeros((1, bad)), np.zeros(1))])
    with pytest.raises(ValueError):                          # three hidden layers
        MLPPolicy.from_layers([(np.zeros((16, 24)), np.zeros(16))] + [(np.zeros((16, 16)), np.zeros(16))] * 2
                              + [(np.zeros((1, 16)), np.zeros(1))])
    with pytest.raises(ValueError):                          # widths that do not chain
        MLPPolicy.from_layers([(np.zeros((16, 24)), np.zeros(16)), (np.zeros((1, 32)), np.zeros(1))])
    with pytest.raises(ValueError):                          # actor too wide for the kernel
        MLPPolicy.from_actor(_actor((256, 256)))
    with pytest.raises(ValueError):                          # different shapes in one population
        MLPPolicy.stack([cases.random_policy(24, 1, (16,), "tanh", 0, 1, 1), cases.random_policy(24, 1, (32,), "tanh", 0, 1, 1)])
    p = cases.random_policy(24, 1, (16,), "tanh", 0, 1, 1)
    with pytest.raises(ValueError):
        p.reference(np.zeros((4, 23), np.float32))
    pop = MLPPolicy.stack([p] * 4)
    pop.check_envs(256)
    for n in (255, 128, 320):                                # 4 policies: whole wavefronts per policy only
        with pytest.raises(ValueError):
            pop.check_envs(n)
    p.check_envs(293)
    d = pop.desc()
    assert (d.n_hidden, list(d.hidden), d.out_activation, d.n_policies, d.struct_size) == (1, [16, 0], 0, 4, 24)


def _fp32_forward(p, obs):
    """The library's arithmetic on the CPU: float32, bias first, inputs in index order, one fmaf each, tanhf or the clamp,
    two roundings — the C restatement of include/salp_vec.h "Policy" (oracle/salp_oracle.c salp_oracle_policy_forward)."""
    u, a, subnormals = ol.policy_forward(p, obs)
    assert subnormals == 0
    return a


@pytest.mark.parametrize("hidden,out", [((32, 32), "tanh"), ((64, 64), "tanh"), ((16,), "tanh"), ((), "clip"), ((16, 64), "tanh"),
                                        ((48, 32), "clip")])
def test_error_bound_covers_an_fp32_evaluation_and_is_not_slack(hidden, out):
    p = cases.random_policy(24, 2, hidden, out, 7, 1.0, 3.0, free_breathing=True)
    obs = np.random.default_rng(5).uniform(-1.2, 1.2, (4000, 24)).astype(np.float32)
    bound, ref = p.error_bound(obs), p.reference(obs)
    err = np.abs(_fp32_forward(p, obs).astype(np.float64) - ref)
    assert bound.shape == ref.shape and (bound > 0).all()
    assert (err <= bound).all(), (err / bound).max()
    assert bound.max() < 1e-4 and bound.min() >= U * np.abs(ref).min()
    # output weights off by 2^-12 relative are far outside it: the bound separates right from nearly right
    W, b = p.layers[-1]
    q = MLPPolicy(p.layers[:-1] + [(W * np.float32(1 + 2.0 ** -12), b)], p.scale, p.shift, p.out)
    assert (np.abs(q.reference(obs) - ref) > bound).mean() > 0.25      # (a saturated clip hides it)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_closed_loop_recipe_on_the_oracle(name):
    cfg, policy, f64, i32, obs_in, actions, outs = cases.oracle_closed_loop(name)
    c = cases.CASES[name]
    assert pc.EXPECT_KERNEL[c["case"]][::2] == c["kernel"] and pc.EXPECT_KERNEL[c["case"]][1] == 3
    assert policy.hidden == tuple(c["hidden"]) and policy.act_dim == cfg.act_dim and policy.obs_dim == cfg.obs_dim == 24
    ev = pc.count_events(outs)
    s = cases.squashed(policy, actions)
    bound = policy.error_bound(obs_in)
    print(f"{name}: {ev}; squashed actions in [{s.min():.3f}, {s.max():.3f}]; error bound max {bound.max():.3g}")
    cases.assert_closed_loop_events(name, ev, policy, actions)
    assert bound.max() < cases.BOUND_CEILING, bound.max()
    # the chain is closed: every action is the policy on the row before it
    assert np.array_equal(obs_in[1:], outs["obs"][:-1])
    if not cfg.forced_breathing:
        assert actions[..., 0].min() >= 0.0 and actions[..., 0].max() <= 1.0
