"""Small MLP policies that run INSIDE the rollout kernel (`salp_vec_rollout_policy`, include/salp_vec.h "Policy").

`MLPPolicy` holds the float32 weights of one policy or of a population of P policies of one shape:
    h = relu(W x + b) per hidden layer;  u = W_last h + b_last;  a = act(u) * scale + shift,   act = tanh | clip to [-1, 1]
which is `sac.Actor.forward(obs, deterministic=True)` (its `[0,1] x [-1,1]` rescale for free breathing included) and,
without hidden layers and with `out="clip"`, the scripted pursuit rule.  Needs numpy only; torch for `from_actor`.

`pack()` is the public weight layout of the C ABI (torch's nn.Linear: per layer W[out][in] row-major, then b[out]; then
scale, shift).  `reference(obs)` evaluates the float32 weights in float64; `error_bound(obs)` bounds how far a correct fp32
evaluation in the library's fixed order may be from it.

`GaussianPolicy` adds the log-std head of `sac.Actor` (salp_policy_create_gaussian): the kernel then SAMPLES the action,
`tanh(mu + exp(log_std) z) * scale + shift`, from the policy's own Philox stream (`noise`) and returns its log-probability
(include/salp_vec.h "Sampled actions"); `reference(obs, z)` / `error_bound(obs, z)` state and bound that computation, and
`sampling_stage(mu, ls_raw, z)` the part of it behind the two heads alone.

`wide=True` (constructors, `from_layers`, `from_actor`, `stack`) asks for the WIDE evaluation scheme of
include/salp_vec_policy_wide.h: 1 or 2 hidden layers of multiples of 32 up to 256 units, evaluated on the matrix cores of
the one-food kernels.  The arithmetic and its order are the same, so `reference` and `error_bound` are too.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

OUT_TANH, OUT_CLIP = 0, 1
_OUT = {"tanh": OUT_TANH, "clip": OUT_CLIP}
MAX_HIDDEN_LAYERS, HIDDEN_STEP, HIDDEN_MAX = 2, 16, 64
WIDE_HIDDEN_STEP, WIDE_HIDDEN_MAX = 32, 256       # the wide scheme (include/salp_vec_policy_wide.h)
U = 2.0 ** -24          # unit roundoff of float32


class CPolicyDesc(ctypes.Structure):
    """salp_policy_desc_t"""
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_hidden", ctypes.c_int32), ("hidden", ctypes.c_int32 * 2),
                ("out_activation", ctypes.c_int32), ("n_policies", ctypes.c_int32)]


def _gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


class MLPPolicy:
    """P >= 1 policies of one shape.  `layers`: [(W [P, out, in], b [P, out]), ...] float32, the last one the output
    layer; `scale`, `shift`: [P, act_dim] float32."""

    def __init__(self, layers: Sequence[Tuple[np.ndarray, np.ndarray]], scale: np.ndarray, shift: np.ndarray, out: str = "tanh",
                 wide: bool = False):
        self.wide = bool(wide)
        if out not in _OUT:
            raise ValueError("out must be 'tanh' or 'clip'")
        if not 1 <= len(layers) <= MAX_HIDDEN_LAYERS + 1:
            raise ValueError("a policy has 0, 1 or 2 hidden layers and one output layer")
        self.out = out
        self.layers: List[Tuple[np.ndarray, np.ndarray]] = []
        P = None
        d = None
        for W, b in layers:
            W = np.ascontiguousarray(W, dtype=np.float32)
            b = np.ascontiguousarray(b, dtype=np.float32)
            if W.ndim != 3 or b.ndim != 2 or W.shape[:2] != b.shape:
                raise ValueError(f"layer shapes must be W [P, out, in], b [P, out]; got {W.shape}, {b.shape}")
            if P is None:
                P = W.shape[0]
            if W.shape[0] != P:
                raise ValueError("every layer must hold the same number of policies")
            if d is not None and W.shape[2] != d:
                raise ValueError(f"layer input width {W.shape[2]} does not follow the previous layer's {d} outputs")
            d = W.shape[1]
            self.layers.append((W, b))
        if self.wide and not self.hidden:
            raise ValueError("a wide policy has 1 or 2 hidden layers")
        step, top = (WIDE_HIDDEN_STEP, WIDE_HIDDEN_MAX) if self.wide else (HIDDEN_STEP, HIDDEN_MAX)
        for h in self.hidden:
            if h % step or not step <= h <= top:
                raise ValueError(f"hidden width {h}: must be a multiple of {step} in [{step}, {top}]")
        self.n_policies = int(P)
        self.obs_dim = int(self.layers[0][0].shape[2])
        self.act_dim = int(self.layers[-1][0].shape[1])
        self.scale = np.ascontiguousarray(scale, dtype=np.float32).reshape(self.n_policies, self.act_dim)
        self.shift = np.ascontiguousarray(shift, dtype=np.float32).reshape(self.n_policies, self.act_dim)

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_layers(cls, layers, scale=None, shift=None, out: str = "tanh", wide: bool = False) -> "MLPPolicy":
        """One policy from [(W [out, in], b [out]), ...]; scale / shift default to 1 / 0."""
        ls = [(np.asarray(W, dtype=np.float32)[None], np.asarray(b, dtype=np.float32)[None]) for W, b in layers]
        A = ls[-1][0].shape[1]
        sc = np.ones(A, np.float32) if scale is None else np.asarray(scale, dtype=np.float32)
        sh = np.zeros(A, np.float32) if shift is None else np.asarray(shift, dtype=np.float32)
        return cls(ls, sc[None], sh[None], out, wide)

    @classmethod
    def from_actor(cls, actor, wide: bool = False) -> "MLPPolicy":
        """The deterministic action of a `sac.Actor` (its mean head, tanh, rescale) whose hidden sizes fit (`wide`: the wide
        scheme's sizes — the default 256 x 256 actor among them)."""
        import torch.nn as nn
        lin = [m for m in actor.body if isinstance(m, nn.Linear)] + [actor.mu]
        layers = [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in lin]
        return cls.from_layers(layers, actor.scale.detach().cpu().numpy(), actor.shift.detach().cpu().numpy(), "tanh", wide)

    @classmethod
    def linear(cls, W, b=None, out: str = "clip", scale=None, shift=None) -> "MLPPolicy":
        """a = act(W x + b) * scale + shift, no hidden layer."""
        W = np.asarray(W, dtype=np.float32)
        b = np.zeros(W.shape[0], np.float32) if b is None else b
        return cls.from_layers([(W, b)], scale, shift, out)

    @classmethod
    def stack(cls, policies: Sequence["MLPPolicy"], wide: Optional[bool] = None) -> "MLPPolicy":
        """A population: the policies of the list (each possibly a population itself), in order.  `wide` None: the first one's."""
        p0 = policies[0]
        for p in policies:
            if (p.hidden, p.obs_dim, p.act_dim, p.out) != (p0.hidden, p0.obs_dim, p0.act_dim, p0.out):
                raise ValueError("stack: every policy must have the same shape and output activation")
        layers = [(np.concatenate([p.layers[l][0] for p in policies]), np.concatenate([p.layers[l][1] for p in policies]))
                  for l in range(len(p0.layers))]
        return cls(layers, np.concatenate([p.scale for p in policies]), np.concatenate([p.shift for p in policies]), p0.out,
                   p0.wide if wide is None else wide)

    # ------------------------------------------------------------------ shape
    @property
    def hidden(self) -> Tuple[int, ...]:
        return tuple(int(W.shape[1]) for W, _ in self.layers[:-1])

    @property
    def words(self) -> int:
        """float32 words of one policy in the public layout (salp_policy_words)."""
        return sum(W.shape[1] * W.shape[2] + W.shape[1] for W, _ in self.layers) + 2 * self.act_dim

    def desc(self) -> CPolicyDesc:
        d = CPolicyDesc()
        d.struct_size = ctypes.sizeof(CPolicyDesc)
        d.n_hidden = len(self.hidden)
        for i, h in enumerate(self.hidden):
            d.hidden[i] = h
        d.out_activation = _OUT[self.out]
        d.n_policies = self.n_policies
        return d

    def pack(self) -> np.ndarray:
        """The public layout, float32 [P, words]."""
        P = self.n_policies
        parts = []
        for W, b in self.layers:
            parts += [W.reshape(P, -1), b]
        parts += [self.scale, self.shift]
        return np.ascontiguousarray(np.concatenate(parts, axis=1), dtype=np.float32)

    def check_envs(self, n_envs: int) -> None:
        """P == 1 serves any n_envs; P > 1 needs whole wavefronts per policy."""
        P = self.n_policies
        if P > 1 and (n_envs % P or (n_envs // P) % 64):
            raise ValueError(f"{P} policies need n_envs % P == 0 and (n_envs / P) % 64 == 0; n_envs = {n_envs}")

    # ------------------------------------------------------------------ evaluation
    def _grouped(self, obs):
        """obs [..., N, obs_dim] -> float64 [P, M, obs_dim] (env i belongs to policy i // (N / P)) and the way back."""
        x = np.asarray(obs)
        if x.shape[-1] != self.obs_dim:
            raise ValueError(f"obs rows have {x.shape[-1]} columns, the policy takes {self.obs_dim}")
        lead, N, P = x.shape[:-2], x.shape[-2], self.n_policies
        self.check_envs(N)
        g = x.astype(np.float64).reshape(-1, P, N // P, self.obs_dim)            # [L, P, G, OD]
        g = np.moveaxis(g, 1, 0).reshape(P, -1, self.obs_dim)                      # [P, L * G, OD]

        def back(a):                                                              # [P, L * G, A] -> [..., N, A]
            a = a.reshape(P, -1, N // P, self.act_dim)
            return np.moveaxis(a, 0, 1).reshape(lead + (N, self.act_dim))
        return g, back

    def _forward(self, x, with_bound: bool):
        """x float64 [P, M, obs_dim].  Returns the float64 actions and (with_bound) the running forward-error bound of an
        fp32 evaluation: per layer gamma_{n+1} (sum |w| |x| + |b|) for the n fused multiply-adds behind the bias, the
        incoming error carried through |W|; relu, tanh and the clamp are 1-Lipschitz; tanhf within 5 ulp; one rounding for
        the multiply by scale and one for the add of shift.  Where the bound needs |x| of a COMPUTED value it takes the
        exact value plus its own bound.  No measured number enters."""
        e = np.zeros_like(x)
        for li, (W, b) in enumerate(self.layers):
            W64, b64 = W.astype(np.float64), b.astype(np.float64)
            y = np.einsum("poi,pmi->pmo", W64, x) + b64[:, None, :]
            if with_bound:
                aW = np.abs(W64)
                mag = np.einsum("poi,pmi->pmo", aW, np.abs(x) + e) + np.abs(b64)[:, None, :]
                e = _gamma(W.shape[2] + 1) * mag + np.einsum("poi,pmi->pmo", aW, e)
            x = np.maximum(y, 0.0) if li + 1 < len(self.layers) else y
        if self.out == "tanh":
            t = np.tanh(x)
            if with_bound:
                e = e + 5.0 * 2.0 * U * (np.abs(t) + e)          # 5 ulp of tanhf: an ulp is at most 2 u |value|
        else:
            t = np.clip(x, -1.0, 1.0)
        sc, sh = self.scale.astype(np.float64)[:, None, :], self.shift.astype(np.float64)[:, None, :]
        a = t * sc + sh
        if with_bound:
            prod = (np.abs(t) + e) * np.abs(sc)                # |computed product| before its rounding
            e_prod = np.abs(sc) * e + U * prod
            e = e_prod + U * (np.abs(a) + e_prod)
        return a, e

    def reference(self, obs) -> np.ndarray:
        """float64 actions [..., N, act_dim] of observations [..., N, obs_dim] under the float32 weights."""
        g, back = self._grouped(obs)
        return back(self._forward(g, False)[0])

    def error_bound(self, obs) -> np.ndarray:
        """float64 [..., N, act_dim]: |fp32 action - reference(obs)| of a correct evaluation stays below this."""
        g, back = self._grouped(obs)
        return back(self._forward(g, True)[1])


# ---------------------------------------------------------------------- the sampling policy (salp_policy_create_gaussian)
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0       # sac.LOG_STD_MIN / MAX (stable-baselines3): the clamp of the log-std head
NOISE_STREAM = 3                            # fourth Philox counter word of the policy noise (0 env draws, 1 / 2 device actions)
# Accuracy of the device library's functions as the bounds below use them: |computed - exact| <= C * 2^-23 * |exact| on
# the ranges the sampling arithmetic reaches (and an exact 0 where the exact value is 0).  Each C is TWICE the largest
# error that the stand-alone probe profiles/micro/math_accuracy_probe.hip measured against float64 on an MI355X (the device
# functions alone, dense grids, no kernel of the library involved; profiles/r07/ab_notes.md) — no ROCm accuracy table is
# installed next to the compiler.  TANHF is the figure `MLPPolicy._forward` has used since the policy kernels exist.
ULP_EXPF = 1.42     # measured 0.7054 on [-80, 2] (2^24 points), doubled
ULP_LOGF = 2.70     # measured 1.3459 on every u1 = k 2^-24, k = 1 .. 2^24, doubled
ULP_SQRTF = 1.0     # measured 0.5000 (correctly rounded) on every -2 logf(u1), doubled
ULP_COSPIF = 1.46   # measured 0.7268 on every 2 u2 = k 2^-23, k = 0 .. 2^24 - 1, doubled
ULP_LOG1PF = 1.05   # measured 0.5246 on [0, 1) (2^24 points) and 2^-e (1 + m 2^-12), e <= 126, doubled
ULP_TANHF = 5.0
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key) -> np.ndarray:
    """Vectorised Philox4x32-10: counter [..., 4], key [..., 2] (broadcast against each other) -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    mask, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c0, np.uint64(_PHILOX_M1) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(_PHILOX_W0)) & mask, (k1 + np.uint64(_PHILOX_W1)) & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _key_words(key) -> Tuple[int, int]:
    """The handle's key: the 64-bit seed (low word, high word), or the two words themselves."""
    if isinstance(key, (tuple, list, np.ndarray)):
        return int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    return int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF


def noise_words(key, env_index, n, stream: int = NOISE_STREAM) -> np.ndarray:
    """The policy-noise blocks, uint32 [..., 4]: Philox4x32-10(counter = (env_lo, env_hi, n mod 2^32, stream), key);
    `env_index` (global) and `n` (noise step) broadcast against each other.  `stream`: the fourth counter word, 3 for the
    block of action components 0 and 1, 4 for the block of component 2 (include/salp_robot_sampled.h)."""
    env = np.asarray(env_index, dtype=np.uint64)
    nn = np.asarray(n).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    env, nn = np.broadcast_arrays(env, nn)
    ctr = np.stack([env & np.uint64(0xFFFFFFFF), env >> np.uint64(32), nn, np.full(env.shape, int(stream), np.uint64)], axis=-1)
    return philox4x32_10(ctr, np.array(_key_words(key), np.uint64))


def normal_from_words(wa, wb) -> np.ndarray:
    """float64 Box-Muller of the definition: u1 = ((wa >> 8) + 1) 2^-24 in (0, 1], u2 = (wb >> 8) 2^-24 in [0, 1),
    z = sqrt(-2 log u1) cos(2 pi u2) (cos(pi x) evaluated with the argument reduced exactly, as cospi does)."""
    u1 = ((np.asarray(wa, np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    k = (np.asarray(wb, np.uint32) >> np.uint32(8)).astype(np.int64)             # u2 = k 2^-24; cos(2 pi u2) by octant of k
    q, r = k >> 22, (k & ((1 << 22) - 1)).astype(np.float64) * 2.0 ** -23          # 2 u2 = q / 2 + r, r in [0, 1/2)
    cr, sr = np.cos(np.pi * r), np.sin(np.pi * r)
    c = np.where(q == 0, cr, np.where(q == 1, -sr, np.where(q == 2, -cr, sr)))
    return np.sqrt(-2.0 * np.log(u1)) * c


class GaussianPolicy(MLPPolicy):
    """P >= 1 tanh-Gaussian policies of one shape (`sac.Actor`): the `MLPPolicy` of the body and the MEAN head — `layers`,
    `reference(obs)` without z, everything a deterministic run uses — plus the log-std head `log_std = (W [P, A, in], b [P, A])`
    on the same last hidden layer."""
    gaussian = True

    def __init__(self, layers, log_std, scale, shift, wide: bool = False):
        super().__init__(layers, scale, shift, "tanh", wide)
        W, b = log_std
        W = np.ascontiguousarray(W, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        if W.shape != self.layers[-1][0].shape or b.shape != self.layers[-1][1].shape:
            raise ValueError(f"the log-std head must have the mean head's shape {self.layers[-1][0].shape}; got {W.shape}, {b.shape}")
        self.log_std = (W, b)

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_layers(cls, layers, log_std, scale=None, shift=None, wide: bool = False) -> "GaussianPolicy":
        """One policy from [(W [out, in], b [out]), ...] (the last one the mean head) and log_std = (W [A, in], b [A])."""
        m = MLPPolicy.from_layers(layers, scale, shift, "tanh", wide)
        return cls(m.layers, (np.asarray(log_std[0], dtype=np.float32)[None], np.asarray(log_std[1], dtype=np.float32)[None]),
                   m.scale, m.shift, wide)

    @classmethod
    def from_actor(cls, actor, wide: bool = False) -> "GaussianPolicy":
        """A `sac.Actor` whose hidden sizes fit: body, `mu`, `log_std`, scale, shift."""
        m = MLPPolicy.from_actor(actor, wide)
        ls = actor.log_std
        return cls(m.layers, (ls.weight.detach().cpu().numpy()[None], ls.bias.detach().cpu().numpy()[None]), m.scale, m.shift, wide)

    @classmethod
    def linear(cls, *a, **k):
        raise TypeError("GaussianPolicy.from_layers builds a policy without hidden layers")

    @classmethod
    def stack(cls, policies: Sequence["GaussianPolicy"], wide: Optional[bool] = None) -> "GaussianPolicy":
        m = MLPPolicy.stack([p.mean_policy() for p in policies], wide)
        return cls(m.layers, (np.concatenate([p.log_std[0] for p in policies]), np.concatenate([p.log_std[1] for p in policies])),
                   m.scale, m.shift, m.wide)

    def mean_policy(self) -> MLPPolicy:
        """The `MLPPolicy` of the same body and mean head: what salp_vec_rollout_policy runs for this policy."""
        return MLPPolicy(self.layers, self.scale, self.shift, "tanh", self.wide)

    # ------------------------------------------------------------------ shape
    @property
    def words(self) -> int:
        """float32 words of one policy in the public Gaussian layout (salp_policy_words_gaussian)."""
        W = self.log_std[0]
        return super().words + W.shape[1] * W.shape[2] + W.shape[1]

    def pack(self) -> np.ndarray:
        """The public layout, float32 [P, words]: hidden layers, W_mu, b_mu, W_ls, b_ls, scale, shift."""
        P = self.n_policies
        parts = []
        for W, b in self.layers:
            parts += [W.reshape(P, -1), b]
        parts += [self.log_std[0].reshape(P, -1), self.log_std[1], self.scale, self.shift]
        return np.ascontiguousarray(np.concatenate(parts, axis=1), dtype=np.float32)

    # ------------------------------------------------------------------ noise
    @staticmethod
    def noise_words(key, env_index, n, stream: int = NOISE_STREAM) -> np.ndarray:
        return noise_words(key, env_index, n, stream)

    def noise(self, key, env_index, n) -> np.ndarray:
        """float64 z [..., act_dim] of the definition (include/salp_vec.h "Randomness", include/salp_robot_sampled.h):
        component j from words (w[2 (j % 2)], w[2 (j % 2) + 1]) of the block of stream word 3 + j // 2 — components 0 and 1
        from block(env, n) of stream 3, component 2 from the first two words of the block of stream 4.  `key`: the handle's
        seed; `env_index` (global) and `n` broadcast."""
        if self.act_dim > 3:
            raise ValueError(f"the noise is defined for up to 3 action components, not {self.act_dim}")
        w = [noise_words(key, env_index, n, NOISE_STREAM + k) for k in range((self.act_dim + 1) // 2)]
        return np.stack([normal_from_words(w[j // 2][..., 2 * (j % 2)], w[j // 2][..., 2 * (j % 2) + 1])
                         for j in range(self.act_dim)], axis=-1)

    # ------------------------------------------------------------------ evaluation
    def _sampled(self, x, z, with_bound: bool):
        """x float64 [P, M, obs_dim], z float64 [P, M, A].  Returns (action, logp, e_action, e_logp): the float64 values of
        the definition and (with_bound) how far a correct fp32 evaluation in the library's order may be from them.  The
        running bound of `_forward` up to both heads (per layer gamma_{n+1} (sum |w| |x| + |b|), the incoming error
        carried through |W|; the clamp is 1-Lipschitz, and exact where the head is beyond it by more than its bound); then
          z:    logf, the exact doubling, sqrtf (which halves a relative error), cospif and one product: relative
          sd:   the error of ls carried through exp — sd (e^{e_ls} - 1) — plus expf's own
          u:    e_mu + e_sd (|z| + e_z) + sd e_z, one rounding of the fma
          a:    tanh is 1-Lipschitz, tanhf's own error, the two roundings of scale / shift
          logp: per component 0.5 e_z (2 |z| + e_z) + e_ls + 2 e_u (the squash term 2 (log 2 - u - softplus(-2u)) has a
                derivative within [-2, 2]), plus the rounding of every operation and library call at its own magnitude.
        Where a magnitude of a COMPUTED value is needed it is the exact one plus its bound.  No measured number but the
        named ULP_* constants enters."""
        e = np.zeros_like(x)
        for W, b in self.layers[:-1]:
            x, e = _affine(W, b, x, e, with_bound)
            x = np.maximum(x, 0.0)
        mu, e_mu = _affine(*self.layers[-1], x, e, with_bound)
        lsr, e_ls = _affine(*self.log_std, x, e, with_bound)
        return self._sampling(mu, e_mu, lsr, e_ls, z, with_bound)

    def _sampling(self, mu, e_mu, lsr, e_ls, z, with_bound: bool):
        """Everything of `_sampled` behind the two heads: mu, lsr (the log-std head before its clamp) and z float64
        [P, M, A]; e_mu, e_ls: how far a computed head may be from them (used with_bound only)."""
        ls = np.clip(lsr, LOG_STD_MIN, LOG_STD_MAX)
        if with_bound:      # a head that is beyond a clamp by more than its own bound leaves the clamp's constant, exactly
            e_ls = np.where((lsr + e_ls < LOG_STD_MIN) | (lsr - e_ls > LOG_STD_MAX), 0.0, e_ls)
        sd = np.exp(ls)
        u = mu + sd * z
        t = np.tanh(u)
        sc, sh = self.scale.astype(np.float64)[:, None, :], self.shift.astype(np.float64)[:, None, :]
        a = t * sc + sh
        m2 = -2.0 * u
        E = np.exp(-np.abs(m2))
        L = np.log1p(E)
        sp = np.maximum(m2, 0.0) + L
        c = (np.log(2.0) - u) - sp
        K = 0.5 * np.log(2.0 * np.pi)
        g1 = -0.5 * z * z
        g2 = g1 - ls
        g3 = g2 - K
        g4 = g3 - 2.0 * c
        logp = g4.sum(axis=-1)
        if not with_bound:
            return a, logp, None, None
        ulp = 2.0 * U
        # z = sqrtf(-2 logf(u1)) * cospif(2 u2): relative errors (1 + r_log)^(1/2) (1 + r_sqrt) (1 + r_cos) (1 + u) - 1
        r_log, r_sqrt, r_cos = ULP_LOGF * ulp, ULP_SQRTF * ulp, ULP_COSPIF * ulp
        r_z = (1.0 + 0.5 * r_log * (1.0 + r_log)) * (1.0 + r_sqrt) * (1.0 + r_cos) * (1.0 + U) - 1.0
        az = np.abs(z)
        e_z = r_z * az
        d_sd = sd * np.expm1(e_ls)
        e_sd = d_sd + ULP_EXPF * ulp * (sd + d_sd)
        e_u = e_mu + e_sd * (az + e_z) + sd * e_z
        e_u = e_u + U * (np.abs(u) + e_u)
        # action
        e_t = e_u + ULP_TANHF * ulp * (np.abs(t) + e_u)
        prod = (np.abs(t) + e_t) * np.abs(sc)
        e_prod = np.abs(sc) * e_t + U * prod
        e_a = e_prod + U * (np.abs(a) + e_prod)
        # log-probability: the inputs' errors through the exact expression, then every operation's own rounding
        e_in = 0.5 * e_z * (2.0 * az + e_z) + e_ls + 2.0 * e_u
        El = np.minimum(1.0, E * np.exp(2.0 * e_u))                       # the largest exp(-|m2|) within the input's error
        Ll = np.log1p(El)
        spl = np.abs(m2) + 2.0 * e_u + Ll
        # expf, carried through log1p (1-Lipschitz); arguments below the probed -80 give results under 2^-115: covered absolutely
        r_E = ULP_EXPF * ulp * El + 2.0 ** -100
        r_L = ULP_LOG1PF * ulp * (Ll + r_E)
        r_sp = r_E + r_L + U * (spl + r_E + r_L)
        r_d = U * np.log(2.0) + U * (np.log(2.0) + np.abs(u) + e_u)        # the constant's rounding, the subtraction's
        mag_c = np.abs(c) + 2.0 * e_u + r_sp + r_d
        r_c = r_sp + r_d + U * mag_c
        r_g1 = 0.5 * U * (az + e_z) ** 2                                   # z * z (the halving is exact)
        mag = np.abs(g1) + 0.5 * e_z * (2.0 * az + e_z) + r_g1
        mag2 = mag + np.abs(ls) + e_ls
        r_g2 = U * mag2
        mag3 = mag2 + r_g2 + K * (1.0 + U)
        r_g3 = U * K + U * mag3
        mag4 = mag3 + r_g3 + 2.0 * mag_c
        r_g4 = U * mag4
        e_g = e_in + r_g1 + r_g2 + r_g3 + 2.0 * r_c + r_g4
        e_logp = e_g.sum(axis=-1)
        if self.act_dim > 1:                                               # the sum of the components: one rounding more each
            e_logp = e_logp + (self.act_dim - 1) * U * (np.abs(g4).sum(axis=-1) + e_logp)
        return a, logp, e_a, e_logp

    def _grouped_z(self, obs, z):
        g, back = self._grouped(obs)
        zz = np.asarray(z, dtype=np.float64)
        x = np.asarray(obs)
        if zz.shape != x.shape[:-1] + (self.act_dim,):
            raise ValueError(f"z must have shape {x.shape[:-1] + (self.act_dim,)}, got {zz.shape}")
        lead, N, P = x.shape[:-2], x.shape[-2], self.n_policies
        gz = np.moveaxis(zz.reshape(-1, P, N // P, self.act_dim), 1, 0).reshape(P, -1, self.act_dim)

        def back1(v):                                                       # [P, L * G] -> [..., N]
            return np.moveaxis(v.reshape(P, -1, N // P), 0, 1).reshape(lead + (N,))
        return g, gz, back, back1

    def reference(self, obs, z=None):
        """Without z: the mean policy's float64 actions (what a deterministic run takes).  With z float64 [..., N, act_dim]:
        (action [..., N, act_dim], logp [..., N]) of the sampling definition in float64 under the float32 weights."""
        if z is None:
            return super().reference(obs)
        g, gz, back, back1 = self._grouped_z(obs, z)
        a, lp, _, _ = self._sampled(g, gz, False)
        return back(a), back1(lp)

    def error_bound(self, obs, z=None):
        """Without z: the mean policy's bound.  With z: (e_action [..., N, act_dim], e_logp [..., N])."""
        if z is None:
            return super().error_bound(obs)
        g, gz, back, back1 = self._grouped_z(obs, z)
        _, _, ea, el = self._sampled(g, gz, True)
        return back(ea), back1(el)

    def sampling_stage(self, mu, ls_raw, z):
        """The sampling arithmetic alone, from GIVEN head values: mu and ls_raw (the log-std head before its clamp)
        [..., N, act_dim] — float32 values, taken as exact — and z float64 of the same shape.  Returns (action, logp,
        e_action, e_logp): the float64 action [..., N, act_dim] and log-probability [..., N] of the definition from those
        heads, and how far a correct fp32 evaluation FROM THE SAME HEADS may be from them.  Nothing is carried in
        (e_mu = e_ls = 0, the clamp is exact); what remains are the terms of `_sampled` behind the heads: expf, the noise's
        logf / sqrtf / cospif, the fma, tanhf, log1pf and the roundings of the logp chain, through the named ULP_* alone."""
        m, r, zz = (np.asarray(v, dtype=np.float64) for v in (mu, ls_raw, z))
        if m.shape[-1] != self.act_dim or r.shape != m.shape or zz.shape != m.shape:
            raise ValueError(f"mu, ls_raw and z must share one shape [..., N, {self.act_dim}]; got {m.shape}, {r.shape}, {zz.shape}")
        lead, N, P, A = m.shape[:-2], m.shape[-2], self.n_policies, self.act_dim
        self.check_envs(N)
        group = lambda v: np.moveaxis(v.reshape(-1, P, N // P, A), 1, 0).reshape(P, -1, A)
        gm = group(m)
        zero = np.zeros_like(gm)
        a, lp, ea, el = self._sampling(gm, zero, group(r), zero, group(zz), True)
        back = lambda v: np.moveaxis(v.reshape(P, -1, N // P, A), 0, 1).reshape(lead + (N, A))
        back1 = lambda v: np.moveaxis(v.reshape(P, -1, N // P), 0, 1).reshape(lead + (N,))
        return back(a), back1(lp), back(ea), back1(el)


def _affine(W, b, x, e, with_bound: bool):
    """y = W x + b in float64 and the running fp32 bound of `MLPPolicy._forward` for one layer."""
    W64, b64 = W.astype(np.float64), b.astype(np.float64)
    y = np.einsum("poi,pmi->pmo", W64, x) + b64[:, None, :]
    if with_bound:
        aW = np.abs(W64)
        mag = np.einsum("poi,pmi->pmo", aW, np.abs(x) + e) + np.abs(b64)[:, None, :]
        e = _gamma(W.shape[2] + 1) * mag + np.einsum("poi,pmi->pmo", aW, e)
    return y, e


# ---------------------------------------------------------------------- evaluation records (salp_vec_evaluate_policy)
EVAL_RETURN, EVAL_FIRST_RETURN, EVAL_FIRST_LENGTH, EVAL_FIRST_END, EVAL_EPISODES, EVAL_FOOD, EVAL_WORDS = 0, 2, 4, 5, 6, 7, 8


def evaluation_views(record) -> dict:
    """Typed views (no copy) of a block of summary records, int32 [N, 8] (numpy array or torch tensor, contiguous):
    `record` itself, `return_sum` and `first_return` float64 [N], `first_length`, `first_end`, `episodes`, `food` int32 [N]
    (include/salp_vec.h SALP_EVAL_*)."""
    if isinstance(record, np.ndarray):
        if record.dtype != np.int32 or record.ndim != 2 or record.shape[1] != EVAL_WORDS or not record.flags.c_contiguous:
            raise ValueError("record must be a contiguous int32 [N, 8] block")
        f64 = record.view(np.float64)                       # [N, 4]
    else:
        import torch
        if record.dtype != torch.int32 or record.dim() != 2 or record.shape[1] != EVAL_WORDS or not record.is_contiguous():
            raise ValueError("record must be a contiguous int32 [N, 8] block")
        f64 = record.view(torch.float64)
    return dict(record=record, return_sum=f64[:, EVAL_RETURN // 2], first_return=f64[:, EVAL_FIRST_RETURN // 2],
                first_length=record[:, EVAL_FIRST_LENGTH], first_end=record[:, EVAL_FIRST_END],
                episodes=record[:, EVAL_EPISODES], food=record[:, EVAL_FOOD])


def summarize_rollout(reward, terminated, truncated, captured=None, record=None) -> np.ndarray:
    """The summary records of a rollout's per-step outputs — the numpy statement of what salp_vec_evaluate_policy leaves:
    reward float32 [H, N], terminated / truncated [H, N] (0 / 1), captured [H, N] (a capture in that step; None: no food
    count).  Returns int32 [N, 8].  The sums are sequential float64 additions of the float32 rewards in step order.
    `record`: records to continue (SALP_EVAL_ACCUMULATE; not modified) — an all-zero record is a fresh one."""
    reward = np.asarray(reward)
    if reward.dtype != np.float32:
        raise ValueError("reward must be float32: the sums are over the float32 values a rollout stores")
    H, N = reward.shape
    term = np.asarray(terminated).astype(bool).reshape(H, N)
    trunc = np.asarray(truncated).astype(bool).reshape(H, N)
    cap = np.zeros((H, N), bool) if captured is None else np.asarray(captured).astype(bool).reshape(H, N)
    rec = np.zeros((N, EVAL_WORDS), np.int32) if record is None else np.array(record, dtype=np.int32, order="C").reshape(N, EVAL_WORDS)
    v = evaluation_views(rec)
    ret, first_ret = v["return_sum"].copy(), v["first_return"].copy()
    first_len, first_end = v["first_length"].copy(), v["first_end"].copy()
    episodes, food = v["episodes"].copy(), v["food"].copy()
    for t in range(H):
        r = reward[t].astype(np.float64)
        ret = ret + r
        open_ = first_end == 0
        first_ret = np.where(open_, first_ret + r, first_ret)
        first_len = first_len + open_.astype(np.int32)
        first_end = np.where(open_, np.where(term[t], 1, np.where(trunc[t], 2, 0)), first_end).astype(np.int32)    # terminated wins
        episodes = episodes + (term[t] | trunc[t]).astype(np.int32)
        food = food + cap[t].astype(np.int32)
    v["return_sum"][:], v["first_return"][:] = ret, first_ret
    v["first_length"][:], v["first_end"][:], v["episodes"][:], v["food"][:] = first_len, first_end, episodes, food
    return rec


# ---------------------------------------------------------------------- robot evaluation records (salp_robot_vec_evaluate_policy)
REVAL_ACCUMULATE, REVAL_FIRST_EPISODE = 4, 8      # call flags next to SALP_DEVICE_PTRS (include/salp_robot_evaluate.h)
(REVAL_RETURN, REVAL_FIRST_RETURN, REVAL_EULER_STEPS, REVAL_FIRST_LENGTH, REVAL_FIRST_END, REVAL_EPISODES, REVAL_REACHED,
 REVAL_FIRST_EULER_STEPS, REVAL_WORDS) = 0, 2, 4, 6, 7, 8, 9, 10, 12


def robot_evaluation_views(record) -> dict:
    """Typed views (no copy) of a block of robot summary records, int32 [N, 12] (numpy array or torch tensor, contiguous):
    `record` itself, `return_sum` and `first_return` float64 [N], `euler_steps` int64 [N], `first_length`, `first_end`,
    `episodes`, `reached`, `first_euler_steps` int32 [N] (include/salp_robot_evaluate.h SALP_REVAL_*)."""
    if isinstance(record, np.ndarray):
        if record.dtype != np.int32 or record.ndim != 2 or record.shape[1] != REVAL_WORDS or not record.flags.c_contiguous:
            raise ValueError("record must be a contiguous int32 [N, 12] block")
        f64, i64 = record.view(np.float64), record.view(np.int64)             # [N, 6]
    else:
        import torch
        if record.dtype != torch.int32 or record.dim() != 2 or record.shape[1] != REVAL_WORDS or not record.is_contiguous():
            raise ValueError("record must be a contiguous int32 [N, 12] block")
        f64, i64 = record.view(torch.float64), record.view(torch.int64)
    return dict(record=record, return_sum=f64[:, REVAL_RETURN // 2], first_return=f64[:, REVAL_FIRST_RETURN // 2],
                euler_steps=i64[:, REVAL_EULER_STEPS // 2], first_length=record[:, REVAL_FIRST_LENGTH],
                first_end=record[:, REVAL_FIRST_END], episodes=record[:, REVAL_EPISODES], reached=record[:, REVAL_REACHED],
                first_euler_steps=record[:, REVAL_FIRST_EULER_STEPS])


def summarize_robot_rollout(reward, terminated, truncated, inner_steps, record=None, first_episode=False) -> np.ndarray:
    """The summary records of a robot rollout's per-step outputs — the numpy statement of what
    salp_robot_vec_evaluate_policy leaves: reward float32 [H, N], terminated / truncated [H, N] (0 / 1), inner_steps
    integer [H, N].  Returns int32 [N, 12].  The float64 sums are sequential additions of the float32 rewards in step order.
    `record`: records to continue (SALP_ROBOT_EVAL_ACCUMULATE; not modified) — an all-zero record is a fresh one.
    `first_episode` (SALP_ROBOT_EVAL_FIRST_EPISODE): a robot's steps after the first ending of its record are ignored."""
    reward = np.asarray(reward)
    if reward.dtype != np.float32:
        raise ValueError("reward must be float32: the sums are over the float32 values a rollout stores")
    H, N = reward.shape
    term = np.asarray(terminated).astype(bool).reshape(H, N)
    trunc = np.asarray(truncated).astype(bool).reshape(H, N)
    inner = np.asarray(inner_steps).astype(np.int64).reshape(H, N)
    rec = np.zeros((N, REVAL_WORDS), np.int32) if record is None else np.array(record, dtype=np.int32, order="C").reshape(N, REVAL_WORDS)
    v = robot_evaluation_views(rec)
    ret, first_ret, euler = v["return_sum"].copy(), v["first_return"].copy(), v["euler_steps"].copy()
    first_len, first_end, first_euler = v["first_length"].copy(), v["first_end"].copy(), v["first_euler_steps"].copy()
    episodes, reached = v["episodes"].copy(), v["reached"].copy()
    for t in range(H):
        r = reward[t].astype(np.float64)
        open_ = first_end == 0
        run = open_ if first_episode else np.ones(N, bool)
        ret = np.where(run, ret + r, ret)
        euler = np.where(run, euler + inner[t], euler)
        first_ret = np.where(open_, first_ret + r, first_ret)
        first_len = first_len + open_.astype(np.int32)
        first_euler = np.where(open_, first_euler + inner[t], first_euler).astype(np.int32)
        first_end = np.where(open_, np.where(term[t], 1, np.where(trunc[t], 2, 0)), first_end).astype(np.int32)    # terminated wins
        episodes = episodes + (run & (term[t] | trunc[t])).astype(np.int32)
        reached = reached + (run & term[t]).astype(np.int32)
    v["return_sum"][:], v["first_return"][:], v["euler_steps"][:] = ret, first_ret, euler
    v["first_length"][:], v["first_end"][:], v["first_euler_steps"][:] = first_len, first_end, first_euler
    v["episodes"][:], v["reached"][:] = episodes, reached
    return rec


# ---------------------------------------------------------------------- navigation records (salp_vec_evaluate_navigation)
(NAV_STEPS, NAV_STATUS, NAV_PATH, NAV_LATERAL, NAV_XMIN, NAV_XMAX, NAV_YMIN, NAV_YMAX, NAV_X, NAV_Y,
 NAV_WORDS) = 0, 1, 2, 4, 6, 8, 10, 12, 14, 16, 20
NAV_REACHED, NAV_COLLIDED, NAV_CAPTURED = 1, 2, 4


def navigation_views(record) -> dict:
    """Typed views (no copy) of a block of navigation records, int32 [N, 20] (numpy array or torch tensor, contiguous):
    `record` itself, `steps` and `status` int32 [N] (status bits NAV_REACHED / NAV_COLLIDED / NAV_CAPTURED), `path_sum`,
    `lateral_sum`, `xmin`, `xmax`, `ymin`, `ymax`, `x`, `y` float64 [N] (include/salp_vec.h SALP_NAV_*)."""
    if isinstance(record, np.ndarray):
        if record.dtype != np.int32 or record.ndim != 2 or record.shape[1] != NAV_WORDS or not record.flags.c_contiguous:
            raise ValueError("record must be a contiguous int32 [N, 20] block")
        f64 = record.view(np.float64)                       # [N, 10]
    else:
        import torch
        if record.dtype != torch.int32 or record.dim() != 2 or record.shape[1] != NAV_WORDS or not record.is_contiguous():
            raise ValueError("record must be a contiguous int32 [N, 20] block")
        f64 = record.view(torch.float64)
    return dict(record=record, steps=record[:, NAV_STEPS], status=record[:, NAV_STATUS], path_sum=f64[:, NAV_PATH // 2],
                lateral_sum=f64[:, NAV_LATERAL // 2], xmin=f64[:, NAV_XMIN // 2], xmax=f64[:, NAV_XMAX // 2],
                ymin=f64[:, NAV_YMIN // 2], ymax=f64[:, NAV_YMAX // 2], x=f64[:, NAV_X // 2], y=f64[:, NAV_Y // 2])


def navigation_line(line, n: int) -> np.ndarray:
    """`line` as float64 [n, 4] (start x, start y, goal x, goal y): one line for every env or one per env."""
    ln = np.asarray(line, np.float64)
    if ln.shape == (4,):
        ln = np.broadcast_to(ln, (n, 4))
    if ln.shape != (n, 4):
        raise ValueError(f"line must be [4] or [{n}, 4] (start x, start y, goal x, goal y)")
    if not np.isfinite(ln).all():
        raise ValueError("line must be finite")
    return np.ascontiguousarray(ln)


def navigation_record(pos, steps, line, goal_radius, collided=None, captured=None, record=None) -> np.ndarray:
    """The navigation records of a path — the numpy statement of what salp_vec_evaluate_navigation leaves: pos float64
    [T + 1, N, 2], pos[0] the position at entry and pos[t] the one after step t; steps [N] (or None = T): the most steps an
    env takes over this piece; line [4] or [N, 4]; collided / captured [T, N] (that step collided / captured; None: no bit).
    An env takes step t while t <= steps and it has not been within `goal_radius` of its goal after a step.  Returns int32
    [N, 20].  The sums are sequential float64 additions in step order, with sqrt and division correctly rounded.
    `record`: records to continue (SALP_EVAL_ACCUMULATE; not modified) — one with steps == 0 and status == 0 is a fresh one,
    one that has reached its goal is returned unchanged."""
    pos = np.asarray(pos)
    if pos.dtype != np.float64 or pos.ndim != 3 or pos.shape[2] != 2 or pos.shape[0] < 1:
        raise ValueError("pos must be float64 [T + 1, N, 2]")
    T, N = pos.shape[0] - 1, pos.shape[1]
    radius = float(goal_radius)
    if not (np.isfinite(radius) and radius > 0.0):
        raise ValueError("goal_radius must be finite and positive")
    ln = navigation_line(line, N)
    cap = np.full(N, T, np.int64) if steps is None else np.asarray(steps).astype(np.int64).reshape(N)
    if (cap < 0).any() or (cap > T).any():
        raise ValueError("steps must be within 0..T")
    col = np.zeros((T, N), bool) if collided is None else np.asarray(collided).astype(bool).reshape(T, N)
    got = np.zeros((T, N), bool) if captured is None else np.asarray(captured).astype(bool).reshape(T, N)
    rec = np.zeros((N, NAV_WORDS), np.int32) if record is None else np.array(record, dtype=np.int32, order="C").reshape(N, NAV_WORDS)
    v = navigation_views(rec)
    fresh = (v["steps"] == 0) & (v["status"] == 0)
    for k, src in (("xmin", pos[0, :, 0]), ("xmax", pos[0, :, 0]), ("ymin", pos[0, :, 1]), ("ymax", pos[0, :, 1]),
                   ("x", pos[0, :, 0]), ("y", pos[0, :, 1]), ("path_sum", 0.0), ("lateral_sum", 0.0)):
        v[k][:] = np.where(fresh, src, v[k])
    rec[:, NAV_WORDS - 2:] = np.where(fresh[:, None], 0, rec[:, NAV_WORDS - 2:])
    sx, sy, gx, gy = ln[:, 0], ln[:, 1], ln[:, 2], ln[:, 3]
    dx, dy = gx - sx, gy - sy
    L = np.sqrt(dx * dx + dy * dy) + 1e-12
    dnx, dny = dx / L, dy / L
    nsteps, status = v["steps"].copy(), v["status"].copy()
    path, lat = v["path_sum"].copy(), v["lateral_sum"].copy()
    xmin, xmax, ymin, ymax = v["xmin"].copy(), v["xmax"].copy(), v["ymin"].copy(), v["ymax"].copy()
    lx, ly = v["x"].copy(), v["y"].copy()
    for t in range(1, T + 1):
        run = ((status & NAV_REACHED) == 0) & (t <= cap)
        if not run.any():
            break
        x, y, px, py = pos[t, :, 0], pos[t, :, 1], pos[t - 1, :, 0], pos[t - 1, :, 1]
        seg = np.sqrt((x - px) * (x - px) + (y - py) * (y - py))
        path = np.where(run, path + seg, path)
        lat = np.where(run, lat + np.abs((x - sx) * dny - (y - sy) * dnx), lat)
        xmin, xmax = np.where(run, np.minimum(xmin, x), xmin), np.where(run, np.maximum(xmax, x), xmax)
        ymin, ymax = np.where(run, np.minimum(ymin, y), ymin), np.where(run, np.maximum(ymax, y), ymax)
        nsteps = nsteps + run.astype(np.int32)
        reached = np.sqrt((x - gx) * (x - gx) + (y - gy) * (y - gy)) < radius
        bits = np.where(col[t - 1], NAV_COLLIDED, 0) | np.where(got[t - 1], NAV_CAPTURED, 0) | np.where(reached, NAV_REACHED, 0)
        status = np.where(run, status | bits, status).astype(np.int32)
        lx, ly = np.where(run, x, lx), np.where(run, y, ly)
    v["steps"][:], v["status"][:], v["path_sum"][:], v["lateral_sum"][:] = nsteps, status, path, lat
    v["xmin"][:], v["xmax"][:], v["ymin"][:], v["ymax"][:], v["x"][:], v["y"][:] = xmin, xmax, ymin, ymax, lx, ly
    return rec


def pursuit_policy(gain: float = 3.0, obs_dim: int = 24) -> MLPPolicy:
    """`navigation_eval.pursuit_policy` as an in-kernel policy: clip(-gain * obs[13], -1, 1)."""
    W = np.zeros((1, obs_dim), np.float32)
    W[0, 13] = -gain
    return MLPPolicy.linear(W, None, out="clip")
