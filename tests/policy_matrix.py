"""The shape x kernel matrix of the in-kernel policy, shared by tests/test_gpu_policy_matrix.py and its CPU guard
tests/test_policy_matrix.py.  Needs numpy, the package's configuration, `policy.MLPPolicy` and the oracle binding — no GPU
library.  Configurations and injected start states are those of tests/parity_cases.py.

What the matrix is for: every policy shape the ABI accepts (0, 1 or 2 hidden layers of 16, 32, 48 or 64 units: 21 shapes),
with both action widths, and the shapes with h0 != h1 in every rollout kernel family, compared with
`oracle_lib.policy_forward` — the arithmetic include/salp_vec.h promises, restated in C from the public weight layout.
For `clip` policies that chain is IEEE arithmetic only, so the comparison is bit for bit; for `tanh` policies everything in
front of tanhf is, and the rest is held to tanhf's 5 ulp and the two final roundings (`tanh_stage_bound`).

Weights are DENSE seeded normal draws scaled by gain / sqrt(fan_in), all distinct and non-zero, so that no two words of the
re-laid device block can be exchanged unnoticed; scale is not 1, shift is not 0, and the two components differ.  The
seeds and gains were picked on the oracle until every entry passes the guard (not blind, episodes end, no subnormals, every
mutant visible): `SEED0`, `GAINS` and `PICKED` below.
"""
import functools
import itertools

import numpy as np

import oracle_lib as ol
import parity_cases as pc
from policy_cases import drive_oracle
from underwater_swimmer_rl_amd.policy import MLPPolicy, U

H = 64                      # compared steps per entry (on the GPU behind one call of horizon 1, tests/test_gpu_policy_matrix.py)
UPDATE_STEPS = 8            # steps run after policy_update
WAVE = pc.WAVE
WIDTHS = (16, 32, 48, 64)
SHAPES = ((),) + tuple((h,) for h in WIDTHS) + tuple(itertools.product(WIDTHS, WIDTHS))
assert len(SHAPES) == 21

# forced breathing: one component; free breathing: the Box is [0, 1] x [-1, 1] and both components stay inside it
SCALE = {1: (0.75,), 2: (0.4375, 0.75)}
SHIFT = {1: (0.125,), 2: (0.5, 0.125)}

SEED0 = 4000                # entry i draws from seed SEED0 + i unless PICKED says otherwise
GAINS = (1.5, 1.5)          # hidden layers, output layer
# the multi-food and run-time-constant kernels: every one runs these shapes (n, hidden, output activation)
FAMILY_CASES = ("sac_gail_F12", "other_physics_F12", "no_respawn_F3", "F3_other_tank", "class_default_F5", "other_tank_F5_free",
                "F16_sixteen_slots", "F16_sixteen_slots_other_tank", "other_tank_F1")
FAMILY_SHAPES = ((128, (64, 64), "clip"), (128, (48, 32), "tanh"), (128, (16, 64), "clip"), (100, (48, 32), "clip"))
# populations of distinct dense policies: parity case, P, n, hidden, output activation
POPULATIONS = (("sac_gail_F12", 3, 192, (48, 32), "tanh"), ("free_breathing", 2, 128, (16, 64), "clip"),
               ("single_food", 4, 256, (), "clip"))
# entries whose default draw failed the guard on the oracle: name -> (seed, hidden gain, output gain)
PICKED = {
    "single_food-16-clip-n128": (4001, 0.7, 0.7),
    "single_food-64-tanh-n128": (4204, 1.5, 1.5),
    "single_food-16x64-tanh-n128": (4008, 1.0, 1.0),
    "single_food-32x16-clip-n128": (5009, 1.5, 1.5),
    "single_food-32x48-clip-n128": (4411, 1.0, 1.0),
    "single_food-48x16-clip-n128": (5013, 1.5, 1.5),
    "single_food-48x32-tanh-n128": (4014, 2.0, 1.0),
    "single_food-64x16-clip-n128": (4217, 1.5, 1.5),
    "single_food-64x48-clip-n128": (4019, 1.0, 1.0),
    "free_breathing-16-tanh-n128": (5422, 2.0, 2.0),
    "free_breathing-32-clip-n128": (4423, 1.0, 1.0),
    "free_breathing-64-clip-n128": (4625, 1.5, 1.5),
    "free_breathing-16x16-tanh-n128": (6026, 2.0, 2.0),
    "free_breathing-16x32-clip-n128": (4227, 1.0, 0.5),
    "free_breathing-16x48-tanh-n128": (4628, 1.0, 0.5),
    "free_breathing-16x64-clip-n128": (4629, 1.5, 1.5),
    "free_breathing-32x16-tanh-n128": (6230, 1.0, 1.0),
    "free_breathing-32x32-clip-n128": (4031, 1.0, 1.0),
    "free_breathing-32x48-tanh-n128": (4632, 1.5, 1.5),
    "free_breathing-32x64-clip-n128": (7000, 1.5, 1.5),
    "free_breathing-48x16-tanh-n128": (5634, 1.5, 1.5),
    "free_breathing-48x32-clip-n128": (4635, 1.5, 1.5),
    "free_breathing-48x48-tanh-n128": (4236, 0.7, 0.7),
    "free_breathing-48x64-clip-n128": (5037, 1.5, 1.5),
    "free_breathing-64x16-tanh-n128": (4238, 1.0, 1.0),
    "free_breathing-64x64-clip-n128": (4841, 1.0, 1.0),
    "sac_gail_F12-64x64-clip-n128": (4242, 1.5, 1.5),
    "other_physics_F12-64x64-clip-n128": (4446, 1.5, 1.5),
    "other_physics_F12-16x64-clip-n128": (4248, 1.5, 1.5),
    "other_physics_F12-48x32-clip-n100": (4449, 1.5, 1.5),
    "F3_other_tank-16x64-clip-n128": (4056, 2.0, 1.0),
    "other_tank_F5_free-64x64-clip-n128": (4062, 2.0, 2.0),
    "other_tank_F5_free-48x32-clip-n100": (4065, 1.0, 0.5),
    "F16_sixteen_slots_other_tank-64x64-clip-n128": (4270, 1.5, 1.5),
    "other_tank_F1-64x64-clip-n128": (4274, 1.5, 1.5),
}
# one entry per kernel family creates its policy from a device weight buffer as well
DEVICE_WEIGHT_ENTRIES = ("single_food-48x32-tanh-n128", "class_default_F5-48x32-clip-n100", "F16_sixteen_slots-16x64-clip-n128")


def _name(case, hidden, out, n, P=1):
    return f"{case}-{'x'.join(map(str, hidden)) or 'linear'}-{out}-n{n}" + (f"-P{P}" if P > 1 else "")


def _entries():
    rows = []
    for i, hidden in enumerate(SHAPES):                 # all 21 shapes, one component, alternating activations
        rows.append(("single_food", 128, hidden, ("tanh", "clip")[i % 2], 1))
    for i, hidden in enumerate(SHAPES):                 # all 21 shapes, two components, the other activation
        rows.append(("free_breathing", 128, hidden, ("clip", "tanh")[i % 2], 1))
    for case in FAMILY_CASES:
        for n, hidden, out in FAMILY_SHAPES:
            rows.append((case, n, hidden, out, 1))
    for case, P, n, hidden, out in POPULATIONS:
        rows.append((case, n, hidden, out, P))
    table = {}
    for i, (case, n, hidden, out, P) in enumerate(rows):
        name = _name(case, hidden, out, n, P)
        seed, gain, out_gain = PICKED.get(name, (SEED0 + i,) + GAINS)
        slots, cap, literal = pc.EXPECT_KERNEL[case]
        assert cap == 3 and name not in table
        table[name] = dict(case=case, n=n, hidden=tuple(hidden), out=out, P=P, seed=seed, gain=gain, out_gain=out_gain,
                           kernel=(slots, literal), predicated=n % WAVE != 0)
    return table


ENTRIES = _entries()
assert all(k in ENTRIES for k in DEVICE_WEIGHT_ENTRIES) and all(k in ENTRIES for k in PICKED)


def dense_policy(obs_dim, act_dim, hidden, out, seed, gain, out_gain):
    """One policy with dense weights: N(0, 1) * gain / sqrt(fan_in), biases N(0, 1) * 0.1; a value that occurs twice in the
    policy (float32 draws do collide among a few thousand) is drawn again until all are distinct and non-zero."""
    rng = np.random.default_rng(seed)
    widths = (obs_dim,) + tuple(hidden) + (act_dim,)
    sigma = []
    for li in range(len(widths) - 1):
        d, h = widths[li], widths[li + 1]
        g = out_gain if li == len(hidden) else gain
        sigma += [np.full(h * d, g / np.sqrt(d)), np.full(h, 0.1)]
    sigma = np.concatenate(sigma)
    flat = (rng.standard_normal(sigma.size) * sigma).astype(np.float32)
    while True:
        _, first = np.unique(flat, return_index=True)
        again = np.ones(flat.size, bool)
        again[first] = False
        again |= flat == 0
        if not again.any():
            break
        flat[again] = (rng.standard_normal(int(again.sum())) * sigma[again]).astype(np.float32)
    layers, o = [], 0
    for li in range(len(widths) - 1):
        d, h = widths[li], widths[li + 1]
        layers.append((flat[o:o + h * d].reshape(h, d), flat[o + h * d:o + h * d + h]))
        o += h * d + h
    return MLPPolicy.from_layers(layers, np.array(SCALE[act_dim], np.float32), np.array(SHIFT[act_dim], np.float32), out)


def entry_cfg(name):
    return pc.case_cfg(ENTRIES[name]["case"])


def entry_policies(name, generation=0):
    """The entry's P policies; `generation=1`: the second weight set of the same shape (for policy_update)."""
    e, cfg = ENTRIES[name], entry_cfg(name)
    return [dense_policy(cfg.obs_dim, cfg.act_dim, e["hidden"], e["out"], e["seed"] + 100000 * generation + 1000 * k, e["gain"], e["out_gain"])
            for k in range(e["P"])]


def entry_policy(name, generation=0):
    ps = entry_policies(name, generation)
    return ps[0] if len(ps) == 1 else MLPPolicy.stack(ps)


def start_snapshot(name):
    """cfg and the injected start state of an entry."""
    e, cfg = ENTRIES[name], entry_cfg(name)
    orc, f64, i32 = pc.start_oracle(cfg, e["n"], pc.ENV_SEED)
    orc.close()
    return e, cfg, f64, i32


def restated(policy, seen):
    """The restatement on the rows `seen` [..., N, obs_dim]: u, a (float32) — with no subnormal on the way."""
    u, a, sub = ol.policy_forward(policy, seen)
    assert sub == 0, f"{sub} subnormal intermediates"
    return u, a


def tanh_stage_bound(policy, u):
    """For a tanh policy and the restatement's u [..., N, act_dim]: the float64 action tanh(u) * scale + shift and how far a
    correct fp32 evaluation FROM THE SAME u may be from it — the tanh term and the two final roundings of
    `MLPPolicy.error_bound` (policy.py `_forward`) with nothing carried in: tanhf within 5 ulp (an ulp is at most 2 u
    |value|), one rounding for the multiply by scale, one for the add of shift."""
    assert policy.out == "tanh"
    P, N, A = policy.n_policies, u.shape[-2], policy.act_dim
    sc = np.repeat(policy.scale.astype(np.float64), N // P, axis=0).reshape(N, A)      # env i runs policy i // (N / P)
    sh = np.repeat(policy.shift.astype(np.float64), N // P, axis=0).reshape(N, A)
    t = np.tanh(u.astype(np.float64))
    a = t * sc + sh
    e = 5.0 * 2.0 * U * np.abs(t)
    prod = (np.abs(t) + e) * np.abs(sc)
    e_prod = np.abs(sc) * e + U * prod
    return a, e_prod + U * (np.abs(a) + e_prod)


@functools.lru_cache(maxsize=None)
def oracle_closed_loop(name):
    """The oracle stepped closed-loop under the restatement from the injected start state: computed once, shared,
    read-only.  obs_in [H, n, OD] is what each action saw; u, a [H, n, A] the restatement's values; outs the oracle's."""
    e, cfg, f64, i32 = start_snapshot(name)
    policy, n = entry_policy(name), e["n"]
    orc = ol.OracleVec(cfg, n, seed=pc.ENV_SEED)
    orc.set_state(f64, i32)

    def act(t, o):
        u, a, sub = ol.policy_forward(policy, o)
        return a, (u, sub)
    obs_in, a, outs, kept = drive_oracle(orc, H, act)
    u, subnormals = np.stack([k[0] for k in kept]), sum(k[1] for k in kept)
    orc.close()
    for arr in (f64, i32, obs_in, u, a, *outs.values()):
        arr.setflags(write=False)
    return dict(e=e, cfg=cfg, policy=policy, f64=f64, i32=i32, obs_in=obs_in, u=u, a=a, outs=outs, subnormals=subnormals)


# ------------------------------------------------------------------------------------------------ the guard's mutants
def layout(policy):
    """Per layer (offset of W, offset of b, out, in) in the public words of one policy; then the offsets of scale, shift."""
    offs, o, d = [], 0, policy.obs_dim
    for h in policy.hidden + (policy.act_dim,):
        offs.append((o, o + h * d, h, d))
        o += h * d + h
        d = h
    return offs, o, o + policy.act_dim


def _fma32(w, x, acc):
    """fmaf on float32 arrays, exactly: the float64 product of two float32 is exact; the float64 sum with `acc` is rounded
    to odd (TwoSum gives the error term), and a round-to-odd value with 53 >= 24 + 2 bits rounds to float32 as the exact
    sum does."""
    p = w.astype(np.float64) * x.astype(np.float64)
    c = acc.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    fix = (err != 0.0) & ((bits & 1) == 0)
    away = (err > 0.0) == (s > 0.0)             # the exact sum lies beyond s, seen from zero
    bits = np.where(fix, np.where(away, bits + 1, bits - 1), bits)
    return bits.view(np.float64).astype(np.float32)


def py_forward(policy, weights, obs, relu=(True, True), descending=False):
    """The restatement once more, in numpy (`_fma32`), with the variants the guard needs: `relu[l]` False leaves the relu
    off hidden layer l; `descending` adds the inputs in descending index order.  obs [L, N, obs_dim]; weights [P, words].
    Returns u and a, float32 [L, N, act_dim]; the tanh of a tanh policy is float32(np.tanh(float64 u)) — not libm's tanhf, so
    only u and the clip chain are comparable with the C restatement in bits."""
    offs, so, sho = layout(policy)
    P, N, A = policy.n_policies, obs.shape[-2], policy.act_dim
    G = N // P
    u = np.empty(obs.shape[:-1] + (A,), np.float32)
    a = np.empty_like(u)
    for k in range(P):
        w = np.asarray(weights, np.float32).reshape(P, -1)[k]
        x = np.ascontiguousarray(obs[:, k * G:(k + 1) * G], np.float32).reshape(-1, policy.obs_dim)
        for li, (Wo, bo, O, I) in enumerate(offs):
            W, b = w[Wo:Wo + O * I].reshape(O, I), w[bo:bo + O]
            acc = np.broadcast_to(b, (x.shape[0], O)).astype(np.float32)
            for i in (range(I - 1, -1, -1) if descending else range(I)):
                acc = _fma32(W[None, :, i], x[:, i:i + 1], acc)
            x = np.maximum(acc, np.float32(0)) if (li + 1 < len(offs) and relu[li]) else acc
        t = np.tanh(x.astype(np.float64)).astype(np.float32) if policy.out == "tanh" else np.minimum(np.maximum(x, np.float32(-1)), np.float32(1))
        v = (t * w[so:so + A]).astype(np.float32) + w[sho:sho + A]
        u[:, k * G:(k + 1) * G] = x.reshape(-1, G, A)
        a[:, k * G:(k + 1) * G] = v.astype(np.float32).reshape(-1, G, A)
    return u, a


def weight_mutants(policy):
    """name -> public weights [P, words] re-indexed the way a wrong device map or a wrong stride in the kernel would read
    them; only the mutants that apply to the policy's shape."""
    w0 = policy.pack()
    offs, so, sho = layout(policy)
    words, A, hid, nh = policy.words, policy.act_dim, policy.hidden, len(policy.hidden)
    out = {}

    def mutant(name):
        out[name] = w0.copy()
        return out[name]

    def columns(Wo, O, I, which):                   # the public words W[j][i], every j, i in `which`
        return np.array([Wo + j * I + i for j in range(O) for i in which])
    if nh == 2 and hid[0] != hid[1]:
        Wo, _, O, I = offs[1]                       # layer 1 read with input stride h1 instead of h0
        j, i = np.meshgrid(np.arange(O), np.arange(I), indexing="ij")
        mutant("layer1_input_stride_h1")[:, (Wo + j * I + i).ravel()] = w0[:, ((Wo + j * hid[1] + i) % words).ravel()]
        if A == 2:
            Wo, _, O, I = offs[2]                   # last-layer rows at stride h0 instead of h1
            j, i = np.meshgrid(np.arange(O), np.arange(I), indexing="ij")
            mutant("last_layer_row_stride_h0")[:, (Wo + j * I + i).ravel()] = w0[:, ((Wo + j * hid[0] + i) % words).ravel()]
    for l in range(nh):                             # the last 16 units of hidden layer l never reach the next layer
        Wo, _, O, I = offs[l + 1]
        mutant(f"hidden{l}_last_chunk_dropped")[:, columns(Wo, O, I, range(I - 16, I))] = 0.0
    Wo, _, O, I = offs[0]
    mutant("inputs_16_23_dropped")[:, columns(Wo, O, I, range(16, 24))] = 0.0
    m = mutant("scale_shift_exchanged")
    m[:, so:so + A], m[:, sho:sho + A] = w0[:, sho:sho + A], w0[:, so:so + A]
    if A == 2:
        bl = offs[-1][1]
        for label, o in (("b_last", bl), ("scale", so), ("shift", sho)):
            mutant(f"component1_takes_component0_{label}")[:, o + 1] = w0[:, o]
    Wo, _, O, I = offs[-1]                          # two weights of one last-layer row, neighbours in one group of 16
    m = mutant("two_weights_swapped_within_a_row")
    m[:, Wo + 1], m[:, Wo + 2] = w0[:, Wo + 2], w0[:, Wo + 1]
    # two weights 16 apart: in the last layer that has more than 16 inputs (the first one has 24)
    Wo, _, O, I = [f for f in offs if f[3] > 16][-1]
    m = mutant("two_weights_swapped_across_chunks")
    m[:, Wo + 2], m[:, Wo + 18] = w0[:, Wo + 18], w0[:, Wo + 2]
    if policy.n_policies > 1:
        out["policy_k_takes_policy_k_minus_1"] = np.roll(w0, 1, axis=0)
    return out


MUTANT_ROWS = 64            # every mutant must change the action on at least this many of the rows it is tried on
MUTANT_STEP_STRIDE = 4      # the mutants are tried on every 4th step's rows (all envs): 16 steps of the 64
