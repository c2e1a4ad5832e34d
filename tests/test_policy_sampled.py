"""`policy.GaussianPolicy` on the CPU: the numpy Philox against the oracle's, the noise definition's ranges and stream
separation, the float64 reference against `sac.Actor.forward` given the same z, the public Gaussian weight layout, and the
recipe guard of the GPU sampled cases (tests/sampled_cases.py): on the oracle alone each case must end episodes the ways
the deterministic cases do, with both error bounds below their ceilings so that the GPU comparison means something."""
import numpy as np
import pytest

import oracle_lib as ol
import parity_cases as pc
import sampled_cases as cases
from underwater_swimmer_rl_amd import policy as pol
from underwater_swimmer_rl_amd.policy import GaussianPolicy, MLPPolicy


def test_numpy_philox_is_the_oracles():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:          # Random123 kat_vectors
        got = pol.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
        assert tuple(int(v) for v in got) == want == tuple(ol.philox(ctr, key))
    rng = np.random.default_rng(0)
    c, k = rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64), rng.integers(0, 2 ** 32, (1000, 2), dtype=np.uint64)
    got = pol.philox4x32_10(c, k)
    assert got.dtype == np.uint32 and got.shape == (1000, 4)
    for i in range(1000):
        assert tuple(int(v) for v in got[i]) == tuple(ol.philox(tuple(int(v) for v in c[i]), tuple(int(v) for v in k[i]))), i


def test_noise_ranges_extremes_and_stream_separation():
    # u1 in (0, 1], u2 in [0, 1): the extreme words
    w = np.array([0, 0xFF, 0x100, 0xFFFFFF00, 0xFFFFFFFF], np.uint32)
    u1 = ((w >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    assert u1.min() == 2.0 ** -24 and u1.max() == 1.0 and u2.min() == 0.0 and u2.max() == 1.0 - 2.0 ** -24
    for wa in (0, 0xFFFFFFFF):
        for wb in (0, 0xFFFFFFFF):
            z = pol.normal_from_words(np.uint32(wa), np.uint32(wb))
            assert np.isfinite(z) and abs(z) <= np.sqrt(48.0 * np.log(2.0)) + 1e-12
    assert pol.normal_from_words(np.uint32(0), np.uint32(0)) == np.sqrt(48.0 * np.log(2.0))          # u1 = 2^-24, u2 = 0
    assert pol.normal_from_words(np.uint32(0xFFFFFFFF), np.uint32(0x12345678)) == 0.0                # u1 = 1
    # the float64 cos(2 pi u2) by exact quarter-turn reduction against the plain expression
    wb = np.random.default_rng(1).integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32)
    plain = np.sqrt(-2.0 * np.log(2.0 ** -24)) * np.cos(2.0 * np.pi * (wb >> np.uint32(8)).astype(np.float64) * 2.0 ** -24)
    assert np.abs(pol.normal_from_words(np.zeros_like(wb), wb) - plain).max() <= 1e-13 * np.sqrt(48.0 * np.log(2.0))
    # a sample of draws: a standard normal (mean, variance, tails) — 2 x 10^5 values
    p = cases.gaussian_policy(24, 2, (16,), 1, 1.0, 1.0, (-1.0, -1.0), free_breathing=True)
    z = p.noise(cases.KEY, np.arange(512, dtype=np.uint64)[None, :], np.arange(200, dtype=np.uint64)[:, None])
    assert z.shape == (200, 512, 2) and z.dtype == np.float64
    assert abs(z.mean()) < 0.01 and abs(z.var() - 1.0) < 0.02 and 0.04 < (np.abs(z) > 2.0).mean() < 0.05
    assert abs(np.corrcoef(z[..., 0].ravel(), z[..., 1].ravel())[0, 1]) < 0.01
    # the stream is its own: the block of (env, n) under counter word 3 is none of the blocks under words 0, 1, 2
    env, n = np.arange(64, dtype=np.uint64)[None, :], np.arange(100, dtype=np.uint64)[:, None]
    mine = pol.noise_words(cases.KEY, env, n)
    key = np.array(pol._key_words(cases.KEY), np.uint64)
    e, nn = np.broadcast_arrays(env, n)
    seen = set(map(bytes, mine.reshape(-1, 4)))
    assert len(seen) == 64 * 100
    for word in (0, 1, 2):
        ctr = np.stack([e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), nn, np.full(e.shape, word, np.uint64)], axis=-1)
        other = pol.philox4x32_10(ctr, key)
        assert not (other == mine).all(axis=-1).any()
        assert not seen & set(map(bytes, other.reshape(-1, 4)))
    # n enters with its low 32 bits; another key gives other draws
    assert np.array_equal(pol.noise_words(cases.KEY, env, n + np.uint64(2 ** 32)), mine)
    assert not np.array_equal(pol.noise_words(cases.KEY + 1, env, n), mine)
    assert np.array_equal(pol.noise_words((cases.KEY, 0), env, n), mine)


def _actor(hidden, act_dim, free, seed):
    import torch
    from underwater_swimmer_rl_amd.sac import Actor
    torch.manual_seed(seed)
    low, high = ([0.0, -1.0], [1.0, 1.0]) if free else (None, None)
    return Actor(24, act_dim, hidden=hidden, act_low=low, act_high=high)


@pytest.mark.parametrize("hidden,act_dim,free", [((32, 32), 1, False), ((16,), 2, True)])
def test_reference_is_the_actors_stochastic_forward_in_float64(hidden, act_dim, free):
    import torch
    actor = _actor(hidden, act_dim, free, seed=4).double()
    p = GaussianPolicy.from_actor(actor.float())
    actor = actor.double()
    rng = np.random.default_rng(0)
    obs = rng.uniform(-1.5, 1.5, (5, 37, 24)).astype(np.float32)
    z = rng.standard_normal((5, 37, act_dim))
    from unittest import mock
    x = torch.from_numpy(obs).double()
    with torch.no_grad(), mock.patch("torch.randn_like", return_value=torch.from_numpy(z)):     # forward's own noise draw
        a, logp = actor(x)
    got_a, got_lp = p.reference(obs, z)
    assert got_a.shape == (5, 37, act_dim) and got_lp.shape == (5, 37) and got_a.dtype == got_lp.dtype == np.float64
    assert np.abs(got_a - a.numpy()).max() <= 1e-12
    assert np.abs(got_lp - logp.numpy()).max() <= 1e-12
    # without z: the mean policy
    assert np.array_equal(p.reference(obs), p.mean_policy().reference(obs))
    assert np.array_equal(p.error_bound(obs), p.mean_policy().error_bound(obs))
    # z = 0 takes the mean action
    a0, _ = p.reference(obs, np.zeros_like(z))
    assert np.array_equal(a0, p.reference(obs))


def test_gaussian_layout_golden_and_mean_sub_block():
    """24 -> 16 -> 1, written out by hand: W0 [16][24], b0 [16], W_mu [1][16], b_mu [1], W_ls [1][16], b_ls [1], scale, shift."""
    W0 = np.arange(16 * 24, dtype=np.float32).reshape(16, 24)
    b0 = 1000.0 + np.arange(16, dtype=np.float32)
    Wm, bm = 2000.0 + np.arange(16, dtype=np.float32)[None], np.array([2500.0], np.float32)
    Wl, bl = 3000.0 + np.arange(16, dtype=np.float32)[None], np.array([3500.0], np.float32)
    p = GaussianPolicy.from_layers([(W0, b0), (Wm, bm)], (Wl, bl), scale=[0.25], shift=[0.75])
    w = p.pack()
    assert p.words == 16 * 24 + 16 + 16 + 1 + 16 + 1 + 2 == 436 and w.shape == (1, 436) and w.dtype == np.float32
    want = np.concatenate([np.arange(384.0), 1000.0 + np.arange(16.0), 2000.0 + np.arange(16.0), [2500.0],
                           3000.0 + np.arange(16.0), [3500.0], [0.25], [0.75]]).astype(np.float32)
    assert np.array_equal(w[0], want)
    m = p.mean_policy()
    assert type(m) is MLPPolicy and m.words == 419 and p.gaussian and not getattr(m, "gaussian", False)
    mw = m.pack()[0]
    assert np.array_equal(mw[:417], w[0, :417]) and np.array_equal(mw[417:], w[0, 434:])       # body + mean head; scale, shift
    d, dm = p.desc(), m.desc()
    assert (d.n_hidden, list(d.hidden), d.out_activation, d.n_policies) == (dm.n_hidden, list(dm.hidden), 0, 1)
    # populations and validation
    pop = GaussianPolicy.stack([p, p])
    assert pop.n_policies == 2 and np.array_equal(pop.pack(), np.concatenate([w, w]))
    with pytest.raises(ValueError):
        GaussianPolicy.from_layers([(W0, b0), (Wm, bm)], (np.zeros((2, 16)), np.zeros(2)))
    with pytest.raises(ValueError):
        p.reference(np.zeros((4, 24), np.float32), np.zeros((4, 2)))
    with pytest.raises(ValueError):
        GaussianPolicy.from_actor(_actor((256, 256), 1, False, 0))


def _fp32_sampled(p, obs, z32):
    """The library's sampling arithmetic restated in numpy float32 on the host (libm in place of the device library; the
    matrix products in float64 rounded once, which is at least as accurate as the fmaf chain)."""
    f = np.float32
    x = obs.astype(np.float64)
    for W, b in p.layers[:-1]:
        x = np.maximum(x @ W[0].astype(np.float64).T + b[0], 0.0).astype(f).astype(np.float64)
    mu = (x @ p.layers[-1][0][0].astype(np.float64).T + p.layers[-1][1][0]).astype(f)
    ls = np.clip((x @ p.log_std[0][0].astype(np.float64).T + p.log_std[1][0]).astype(f), f(-20), f(2))
    sd = np.exp(ls)
    u = (sd.astype(np.float64) * z32 + mu).astype(f)               # one rounding: the fma
    a = np.tanh(u) * p.scale[0] + p.shift[0]
    m2 = f(-2) * u
    sp = np.maximum(m2, f(0)) + np.log1p(np.exp(-np.abs(m2)))
    c = (f(0.693147180559945309) - u) - sp
    g = f(-0.5) * (z32 * z32)
    g = g - ls
    g = g - f(0.918938533204672742)
    g = g - f(2) * c
    lp = g[..., 0] if g.shape[-1] == 1 else g[..., 0] + g[..., 1]
    assert a.dtype == lp.dtype == f
    return a, lp


@pytest.mark.parametrize("hidden,b_ls", [((32, 32), (-1.0, -2.5)), ((), (0.0, -3.0)), ((64, 64), (3.0, -25.0))])
def test_error_bound_covers_an_fp32_evaluation_and_is_not_slack(hidden, b_ls):
    p = cases.gaussian_policy(24, 2, hidden, 7, 1.0, 2.0, b_ls, free_breathing=True)
    rng = np.random.default_rng(5)
    obs = rng.uniform(-1.2, 1.2, (4000, 24)).astype(np.float32)
    z = p.noise(3, np.arange(4000, dtype=np.uint64), np.uint64(17))
    (ra, rl), (ea, el) = p.reference(obs, z), p.error_bound(obs, z)
    a, lp = _fp32_sampled(p, obs, z.astype(np.float32))
    # the host's float32 z is the float64 one rounded once: inside e_z, as the device's is
    assert ea.shape == ra.shape and el.shape == rl.shape and (ea > 0).all() and (el > 0).all()
    assert (np.abs(a - ra) <= ea).all(), (np.abs(a - ra) / ea).max()
    assert (np.abs(lp - rl) <= el).all(), (np.abs(lp - rl) / el).max()
    assert ea.max() < cases.BOUND_CEILING and el.max() < 2 * cases.LOGP_BOUND_CEILING_PER_COMPONENT
    # a log-std bias off by 2^-10 moves logp far outside its bound (and the action, where the head is not clamped)
    W, b = p.log_std
    q = GaussianPolicy(p.layers, (W, b + np.float32(2.0 ** -10)), p.scale, p.shift)
    qa, ql = q.reference(obs, z)
    if max(b_ls) <= 2.0 and min(b_ls) >= -20.0:
        assert (np.abs(ql - rl) > el).mean() > 0.9
        assert (np.abs(qa - ra) > ea).mean() > 0.25
    else:           # beyond the clamps the head is a constant: the same bits
        assert np.array_equal(qa, ra) and np.array_equal(ql, rl)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_sampled_closed_loop_recipe_on_the_oracle(name):
    cfg, policy, f64, i32, z, obs_in, actions, logp, outs = cases.oracle_closed_loop(name)
    c = cases.CASES[name]
    assert pc.EXPECT_KERNEL[c["case"]][::2] == c["kernel"] and pc.EXPECT_KERNEL[c["case"]][1] == 3
    assert policy.hidden == tuple(c["hidden"]) and policy.act_dim == cfg.act_dim and policy.obs_dim == cfg.obs_dim == 24
    ev = pc.count_events(outs)
    ea, el = policy.error_bound(obs_in, z)
    share = cases.off_by_one_share(policy, obs_in, actions)
    print(f"{name}: {ev}; bounds: action {ea.max():.3g}, logp {el.max():.3g}; logp in [{logp.min():.3f}, {logp.max():.3f}]; "
          f"off-by-one share {share:.3f}")
    cases.assert_closed_loop_events(name, ev)
    assert ea.max() < cases.BOUND_CEILING, ea.max()
    assert el.max() < cfg.act_dim * cases.LOGP_BOUND_CEILING_PER_COMPONENT, el.max()
    assert share > cases.OFF_BY_ONE_SHARE
    # the chain is closed: every action is the sample on the row before it
    assert np.array_equal(obs_in[1:], outs["obs"][:-1])
    if not cfg.forced_breathing:
        assert actions[..., 0].min() >= 0.0 and actions[..., 0].max() <= 1.0
    # the log-std head where the table says: about [-3, 0] — or beyond both clamps, by more than the head's weights can undo
    x = obs_in.astype(np.float64)
    for W, b in policy.layers[:-1]:
        x = np.maximum(x @ W[0].astype(np.float64).T + b[0], 0.0)
    wh = x @ policy.log_std[0][0].astype(np.float64).T
    assert np.abs(wh).max() < 4.0
    ls = wh + policy.log_std[1][0]
    if name == "free_breathing_mlp32_clamped":
        assert ls[..., 0].min() > 2.0 and ls[..., 1].max() < -20.0
        assert list(cases.floor_clamped_components(policy)) == [1]
        # ... so the nozzle takes its mean action, whatever the noise
        assert np.abs(actions[..., 1] - policy.mean_policy().reference(obs_in)[..., 1]).max() < 1e-7
    else:
        assert -3.6 < ls.min() and ls.max() < 0.6 and cases.floor_clamped_components(policy).size == 0
