"""What the env shims (vector_env.py, robot_env.py) share.  The array backend: device tensors with `output="torch"`, host
numpy arrays with `output="numpy"`; PyTorch is used for device buffers and streams only.  The policy cache: an env's
in-kernel policies by policy object."""
from __future__ import annotations

import numpy as np

from ._capi import SALP_DEVICE_PTRS, SalpError


def device_index(device) -> int:
    """The HIP ordinal of "cuda:3" (3), 3 (3) or "cuda" (0)."""
    if isinstance(device, str):
        return int(device.split(":")[1]) if ":" in device else 0
    return int(device)


class ArrayBackend:
    """Mixin: `_init_arrays(output, index)` sets `_torch` (the module, or None for numpy) and `device`."""

    def _init_arrays(self, output: str, index: int):
        self._torch, self.device = None, None
        if output == "torch":
            import torch
            if not torch.cuda.is_available():
                raise SalpError("output='torch' needs a ROCm GPU visible to PyTorch")
            self._torch, self.device = torch, torch.device("cuda", index)

    def _empty(self, shape, dtype):
        if self._torch is None:
            return np.empty(shape, dtype)
        return self._torch.empty(shape, dtype=getattr(self._torch, np.dtype(dtype).name), device=self.device)

    @property
    def _flags(self) -> int:
        return SALP_DEVICE_PTRS if self._torch is not None else 0

    @property
    def _stream(self) -> int:
        return 0 if self._torch is None else int(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _actions_in(self, actions, shape):
        """`actions` as a contiguous float32 block of `shape` on this backend."""
        t = self._torch
        if t is None:
            return np.ascontiguousarray(np.asarray(actions, dtype=np.float32).reshape(shape))
        if not isinstance(actions, t.Tensor):
            actions = t.as_tensor(np.asarray(actions, dtype=np.float32))
        return actions.to(device=self.device, dtype=t.float32).reshape(shape).contiguous()

    def _mask_in(self, mask):
        """A reset mask (None, list, array or tensor) as contiguous bytes on this backend."""
        if mask is None:
            return None
        if self._torch is None:
            return np.ascontiguousarray(mask, dtype=np.uint8)
        return self._torch.as_tensor(mask).to(device=self.device, dtype=self._torch.uint8).contiguous()

    def _bool_view(self, flag_bytes):
        """Zero-copy bool view of a buffer of 0 / 1 bytes."""
        return flag_bytes.view(np.bool_ if self._torch is None else self._torch.bool)

    def _is_block(self, x, shape, dtype) -> bool:
        """Is `x` a contiguous block of that dtype and shape where a kernel of this env can take it: on this GPU for a
        torch env, on the host for a numpy env?"""
        t = self._torch
        if t is None:
            return isinstance(x, np.ndarray) and x.dtype == dtype and x.shape == tuple(shape) and x.flags.c_contiguous
        return (isinstance(x, t.Tensor) and x.device == self.device and x.dtype == getattr(t, np.dtype(dtype).name)
                and tuple(x.shape) == tuple(shape) and x.is_contiguous())

    def _out_block(self, out, shape, dtype):
        """A caller's `out` block (None: a new one) for a kernel to write into; refuses one of the other backend, on
        another device or of another shape (the caller's views check dtype and contiguity)."""
        if out is None:
            return self._empty(shape, dtype)
        if self._torch is not None:        # the pointer goes to the kernel as a device pointer: it must be one, on this GPU
            if not isinstance(out, self._torch.Tensor) or out.device != self.device:
                raise ValueError(f"out must be a torch tensor on {self.device}")
        elif not isinstance(out, np.ndarray):
            raise ValueError("out must be a numpy array (this env returns host arrays)")
        if tuple(out.shape) != tuple(shape):
            raise ValueError(f"out must be an {np.dtype(dtype).name} [{shape[0]}, {shape[1]}] block")
        return out


class PolicyCache:
    """Mixin: the in-kernel policies of an env.  The env names the handle class of its library (`_handle_class`), keeps
    `_policy_cache` (id(policy object) -> (policy object, its handle)) and makes handles in `make_policy`."""
    _handle_class = None

    def _check_policy(self, policy):
        """What `make_policy` checks of a policy object before the library sees it."""
        if (policy.obs_dim, policy.act_dim) != (self.obs_dim, self.act_dim):
            raise ValueError(f"the policy maps {policy.obs_dim} -> {policy.act_dim}, this env {self.obs_dim} -> {self.act_dim}")
        policy.check_envs(self.num_envs)

    def _policy_handle(self, policy):
        """`policy` if it is a handle, else the handle made for that policy object at its first use (kept until close())."""
        if isinstance(policy, self._handle_class):
            return policy
        if id(policy) not in self._policy_cache:
            self._policy_cache[id(policy)] = (policy, self.make_policy(policy))
        return self._policy_cache[id(policy)][1]
