"""Small MLP policies that run INSIDE the rollout kernel (`salp_vec_rollout_policy`, include/salp_vec.h "Policy").

`MLPPolicy` holds the float32 weights of one policy or of a population of P policies of one shape:
    h = relu(W x + b) per hidden layer;  u = W_last h + b_last;  a = act(u) * scale + shift,   act = tanh | clip to [-1, 1]
which is `sac.Actor.forward(obs, deterministic=True)` (its `[0,1] x [-1,1]` rescale for free breathing included) and,
without hidden layers and with `out="clip"`, the scripted pursuit rule.  Needs numpy only; torch for `from_actor`.

`pack()` is the public weight layout of the C ABI (torch's nn.Linear: per layer W[out][in] row-major, then b[out]; then
scale, shift).  `reference(obs)` evaluates the float32 weights in float64; `error_bound(obs)` bounds how far a correct fp32
evaluation in the library's fixed order may be from it.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

OUT_TANH, OUT_CLIP = 0, 1
_OUT = {"tanh": OUT_TANH, "clip": OUT_CLIP}
MAX_HIDDEN_LAYERS, HIDDEN_STEP, HIDDEN_MAX = 2, 16, 64
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

    def __init__(self, layers: Sequence[Tuple[np.ndarray, np.ndarray]], scale: np.ndarray, shift: np.ndarray, out: str = "tanh"):
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
        for h in self.hidden:
            if h % HIDDEN_STEP or not HIDDEN_STEP <= h <= HIDDEN_MAX:
                raise ValueError(f"hidden width {h}: must be a multiple of {HIDDEN_STEP} in [{HIDDEN_STEP}, {HIDDEN_MAX}]")
        self.n_policies = int(P)
        self.obs_dim = int(self.layers[0][0].shape[2])
        self.act_dim = int(self.layers[-1][0].shape[1])
        self.scale = np.ascontiguousarray(scale, dtype=np.float32).reshape(self.n_policies, self.act_dim)
        self.shift = np.ascontiguousarray(shift, dtype=np.float32).reshape(self.n_policies, self.act_dim)

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_layers(cls, layers, scale=None, shift=None, out: str = "tanh") -> "MLPPolicy":
        """One policy from [(W [out, in], b [out]), ...]; scale / shift default to 1 / 0."""
        ls = [(np.asarray(W, dtype=np.float32)[None], np.asarray(b, dtype=np.float32)[None]) for W, b in layers]
        A = ls[-1][0].shape[1]
        sc = np.ones(A, np.float32) if scale is None else np.asarray(scale, dtype=np.float32)
        sh = np.zeros(A, np.float32) if shift is None else np.asarray(shift, dtype=np.float32)
        return cls(ls, sc[None], sh[None], out)

    @classmethod
    def from_actor(cls, actor) -> "MLPPolicy":
        """The deterministic action of a `sac.Actor` (its mean head, tanh, rescale) whose hidden sizes fit."""
        import torch.nn as nn
        lin = [m for m in actor.body if isinstance(m, nn.Linear)] + [actor.mu]
        layers = [(m.weight.detach().cpu().numpy(), m.bias.detach().cpu().numpy()) for m in lin]
        return cls.from_layers(layers, actor.scale.detach().cpu().numpy(), actor.shift.detach().cpu().numpy(), "tanh")

    @classmethod
    def linear(cls, W, b=None, out: str = "clip", scale=None, shift=None) -> "MLPPolicy":
        """a = act(W x + b) * scale + shift, no hidden layer."""
        W = np.asarray(W, dtype=np.float32)
        b = np.zeros(W.shape[0], np.float32) if b is None else b
        return cls.from_layers([(W, b)], scale, shift, out)

    @classmethod
    def stack(cls, policies: Sequence["MLPPolicy"]) -> "MLPPolicy":
        """A population: the policies of the list (each possibly a population itself), in order."""
        p0 = policies[0]
        for p in policies:
            if (p.hidden, p.obs_dim, p.act_dim, p.out) != (p0.hidden, p0.obs_dim, p0.act_dim, p0.out):
                raise ValueError("stack: every policy must have the same shape and output activation")
        layers = [(np.concatenate([p.layers[l][0] for p in policies]), np.concatenate([p.layers[l][1] for p in policies]))
                  for l in range(len(p0.layers))]
        return cls(layers, np.concatenate([p.scale for p in policies]), np.concatenate([p.shift for p in policies]), p0.out)

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


def pursuit_policy(gain: float = 3.0, obs_dim: int = 24) -> MLPPolicy:
    """`navigation_eval.pursuit_policy` as an in-kernel policy: clip(-gain * obs[13], -1, 1)."""
    W = np.zeros((1, obs_dim), np.float32)
    W[0, 13] = -gain
    return MLPPolicy.linear(W, None, out="clip")
