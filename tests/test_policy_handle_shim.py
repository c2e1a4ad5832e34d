"""The Python side of a policy object: one handle class behind `_capi.PolicyHandle` (salp_policy_*) and
`robot_env.RobotPolicyHandle` (salp_robot_policy_*), one policy cache behind both envs.  A stub stands in for the ctypes
library and records every call, so what each method hands to which function — and the defaults the two classes keep for
themselves — is checked without a GPU and without torch."""
import ctypes

import numpy as np
import pytest

from underwater_swimmer_rl_amd import _capi, navigation_eval
from underwater_swimmer_rl_amd.policy import MLPPolicy
from underwater_swimmer_rl_amd.robot_env import RobotPolicyHandle, SalpRobotVectorEnv
from underwater_swimmer_rl_amd.vector_env import SalpVectorEnv

ENV_STREAM = 0x5EA0          # what the stub owner reports as its current stream
POINTER = 0xB10C             # the policy's address


class StubLib:
    """Every attribute is a function that records (name, args) and returns `rc`; the two error strings are bytes."""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return {"salp_last_error": b"snake says no", "salp_robot_last_error": b"robot says no"}.get(name, self.rc)
        return f


class StubOwner:
    """What a handle needs of the SalpLib / the env that made it."""
    _stream = ENV_STREAM

    def __init__(self, rc=0):
        self.lib = self.L = StubLib(rc)
        self._policies = []


class DeviceBlock:
    """Stands for a device tensor: it has data_ptr()."""

    def data_ptr(self):
        return 0xD0D0


HANDLES = [(_capi.PolicyHandle, "salp_policy_"), (RobotPolicyHandle, "salp_robot_policy_")]


def make(cls, rc=0):
    owner = StubOwner(rc)
    h = cls(owner, ctypes.c_void_p(POINTER), 2, 77, True)
    owner._policies.append(h)
    return owner, h


@pytest.mark.parametrize("cls,prefix", HANDLES)
def test_a_handle_records_what_it_was_made_with(cls, prefix):
    owner, h = make(cls)
    assert (h.owner, h._p.value, h.n_policies, h.words, h.gaussian) == (owner, POINTER, 2, 77, True)
    assert cls(owner, ctypes.c_void_p(), 1, 5).gaussian is False       # (a NULL policy: nothing to destroy)
    assert owner.lib.calls == []
    h._p = ctypes.c_void_p()      # (nothing to destroy when the stubs go)


def test_the_robot_handle_still_names_its_env():
    owner, h = make(RobotPolicyHandle)
    assert h.env is owner


@pytest.mark.parametrize("cls,prefix", HANDLES)
def test_noise_step_reads_through_its_own_library(cls, prefix):
    owner, h = make(cls)
    assert h.noise_step == 0           # the stub writes nothing into the uint64
    (name, args), = owner.lib.calls
    assert name == prefix + "noise_step" and len(args) == 2 and args[0] is h._p
    assert type(args[1]) is type(ctypes.byref(ctypes.c_uint64()))


@pytest.mark.parametrize("cls,prefix", HANDLES)
def test_set_noise_step_masks_to_64_bits_and_passes_the_stream(cls, prefix):
    owner, h = make(cls)
    h.set_noise_step(-1, 12)
    h.set_noise_step(2 ** 64 + 5, 12)
    h.set_noise_step(7)
    default_stream = ENV_STREAM if cls is RobotPolicyHandle else 0       # the robot's default: its env's current stream
    assert owner.lib.calls == [(prefix + "set_noise_step", (h._p, 0xFFFFFFFFFFFFFFFF, 12)),
                               (prefix + "set_noise_step", (h._p, 5, 12)),
                               (prefix + "set_noise_step", (h._p, 7, default_stream))]


@pytest.mark.parametrize("cls,prefix", HANDLES)
def test_update_passes_weights_flags_stream_in_this_order(cls, prefix):
    owner, h = make(cls)
    w = np.zeros((2, 77), np.float32)
    h.update(w, 1, 9)
    assert owner.lib.calls == [(prefix + "update", (h._p, w.ctypes.data, 1, 9))]


def test_update_defaults_of_the_snake_handle():
    owner, h = make(_capi.PolicyHandle)
    w, dev = np.zeros((2, 77), np.float32), DeviceBlock()
    h.update(w)
    h.update(dev)                      # no detection: flags stay 0 unless given
    assert owner.lib.calls == [("salp_policy_update", (h._p, w.ctypes.data, 0, 0)), ("salp_policy_update", (h._p, 0xD0D0, 0, 0))]


def test_update_defaults_of_the_robot_handle():
    owner, h = make(RobotPolicyHandle)
    w, dev = np.zeros((2, 77), np.float32), DeviceBlock()
    h.update(w)                        # flags=None: a numpy array is a host pointer
    h.update(dev)                      # ... a device tensor sets SALP_DEVICE_PTRS
    h.update(dev, flags=0, stream=3)
    assert owner.lib.calls == [("salp_robot_policy_update", (h._p, w.ctypes.data, 0, ENV_STREAM)),
                               ("salp_robot_policy_update", (h._p, 0xD0D0, _capi.SALP_DEVICE_PTRS, ENV_STREAM)),
                               ("salp_robot_policy_update", (h._p, 0xD0D0, 0, 3))]


@pytest.mark.parametrize("cls,prefix", HANDLES)
def test_close_destroys_once_and_leaves_the_owner(cls, prefix):
    owner, h = make(cls)
    p = h._p
    h.close()
    assert owner.lib.calls == [(prefix + "destroy", (p,))] and owner._policies == [] and not h._p
    h.close()
    h.__del__()
    assert len(owner.lib.calls) == 1


@pytest.mark.parametrize("cls,prefix,error,names", [
    (_capi.PolicyHandle, "salp_policy_", "snake says no",
     ("salp_policy_noise_step", "salp_policy_set_noise_step", "salp_policy_update")),
    (RobotPolicyHandle, "salp_robot_policy_", "robot says no", ("noise_step", "set_noise_step", "policy update"))])
def test_a_failure_quotes_its_own_library(cls, prefix, error, names):
    owner, h = make(cls, rc=-1)
    for name, call in zip(names, (lambda: h.noise_step, lambda: h.set_noise_step(1), lambda: h.update(np.zeros(1, np.float32)))):
        with pytest.raises(_capi.SalpError) as e:
            call()
        assert str(e.value) == f"{name} failed (-1): {error}"
    h._p = ctypes.c_void_p()


def test_the_two_handle_classes_stay_apart():
    assert not issubclass(RobotPolicyHandle, _capi.PolicyHandle) and not issubclass(_capi.PolicyHandle, RobotPolicyHandle)
    import underwater_swimmer_rl_amd as pkg
    assert pkg.RobotPolicyHandle is RobotPolicyHandle and pkg.PolicyHandle is _capi.PolicyHandle
    _, robot = make(RobotPolicyHandle)
    with pytest.raises(TypeError, match="MLPPolicy .* or a policy handle"):      # before any env is made
        navigation_eval.run_navigation_trials_in_kernel(robot, num_trials=1)
    robot._p = ctypes.c_void_p()


@pytest.mark.parametrize("env_cls,own,other,dims", [(SalpVectorEnv, _capi.PolicyHandle, RobotPolicyHandle, (24, 1)),
                                                    (SalpRobotVectorEnv, RobotPolicyHandle, _capi.PolicyHandle, (6, 3))])
def test_an_env_takes_its_own_handles_and_caches_one_per_policy_object(env_cls, own, other, dims):
    env = object.__new__(env_cls)          # no library, no GPU: only what the policy cache reads
    env._h, env._policy_cache, env.num_envs = None, {}, 128
    env.obs_dim, env.act_dim = dims
    made = []
    _, mine = make(own)
    _, foreign = make(other)
    # its own handle goes through as it is; the other library's handle is no handle here: it is taken for a policy
    # object, and make_policy's dimension check finds none of a policy's attributes on it
    assert env._policy_handle(mine) is mine and env._policy_cache == {}
    with pytest.raises(AttributeError, match="obs_dim"):
        env._policy_handle(foreign)
    assert env._policy_cache == {}
    # a policy object: make_policy once, then the cached handle
    env.make_policy = lambda policy: made.append(policy) or mine
    pol = MLPPolicy.linear(np.zeros((dims[1], dims[0]), np.float32))
    assert env._policy_handle(pol) is mine and env._policy_handle(pol) is mine and made == [pol]
    assert env._policy_cache == {id(pol): (pol, mine)}
    # the check that opens make_policy: dimensions, then whole wavefronts per policy
    wrong = MLPPolicy.linear(np.zeros((dims[1] + 1, dims[0]), np.float32))
    with pytest.raises(ValueError, match=f"the policy maps {dims[0]} -> {dims[1] + 1}, this env {dims[0]} -> {dims[1]}"):
        env_cls.make_policy(env, wrong)
    env.num_envs = 96
    with pytest.raises(ValueError, match="2 policies need n_envs % P == 0"):
        env_cls.make_policy(env, MLPPolicy.stack([pol, pol]))
    mine._p = foreign._p = ctypes.c_void_p()
