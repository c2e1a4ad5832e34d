"""The robot evaluation calls (salp_robot_vec_evaluate_policy, salp_robot_vec_evaluate_policy_sampled) — the part that
needs no GPU: what check_evaluate_args() of csrc/salp_robot_params.h refuses and with which message, the flag combinations
it accepts, and the constants of include/salp_robot_evaluate.h against policy.py's (tests/robot_evaluate_host_lib.py)."""
import subprocess

import pytest

import native_lib
import robot_evaluate_host_lib as re_
from underwater_swimmer_rl_amd import _capi, policy

INVALID = -1                    # SALP_ERR_INVALID (include/salp_vec.h)
STEPS = 1461                    # robot_max_steps(0.01)


def test_constants_equal_policy_py():
    f = re_.flags()
    assert f == dict(DEVICE_PTRS=_capi.SALP_DEVICE_PTRS, ACCUMULATE=policy.REVAL_ACCUMULATE, FIRST_EPISODE=policy.REVAL_FIRST_EPISODE)
    assert f["ACCUMULATE"] == _capi.EVAL_ACCUMULATE == 4 and f["FIRST_EPISODE"] == 8
    w = re_.words()
    assert w == {k: getattr(policy, "REVAL_" + k) for k in re_.WORD_NAMES}
    assert w["WORDS"] == 12 and w["RETURN"] % 2 == 0 and w["FIRST_RETURN"] % 2 == 0 and w["EULER_STEPS"] % 2 == 0
    # every word but the last belongs to exactly one field
    used = sorted([w["RETURN"], w["RETURN"] + 1, w["FIRST_RETURN"], w["FIRST_RETURN"] + 1, w["EULER_STEPS"], w["EULER_STEPS"] + 1,
                   w["FIRST_LENGTH"], w["FIRST_END"], w["EPISODES"], w["REACHED"], w["FIRST_EULER_STEPS"]])
    assert used == list(range(11))


@pytest.mark.parametrize("flags", [0, 1, 4, 5, 8, 9, 12, 13])
def test_accepted_flag_combinations(flags):
    for H in (1, 7, 1024):
        assert re_.check_evaluate(STEPS, H, flags=flags) == (0, "")
    assert re_.check_evaluate(STEPS, 7, flags=flags, sampled=True, gaussian=True) == (0, "")
    assert re_.check_evaluate(STEPS, 7, flags=flags, gaussian=True) == (0, ""), "a Gaussian policy's mean is evaluated"


def test_a_host_record_needs_no_alignment():
    assert re_.check_evaluate(STEPS, 7, flags=4, rec=0x1004) == (0, "")
    assert re_.check_evaluate(STEPS, 7, flags=5, rec=0x1010) == (0, "")


@pytest.mark.parametrize("kwargs, text", [
    (dict(rec=0), "rec is NULL"),
    (dict(horizon=0), "horizon must be in [1, 1024]"),
    (dict(horizon=-3), "horizon must be in [1, 1024]"),
    (dict(horizon=1025), "horizon must be in [1, 1024]"),
    (dict(flags=2), "unknown flag bits"),
    (dict(flags=16), "unknown flag bits"),
    (dict(flags=0x8000000D), "unknown flag bits"),
    (dict(flags=1, rec=0x1008), "device rec must be 16-byte aligned"),
    (dict(flags=13, rec=0x1004), "device rec must be 16-byte aligned"),
    (dict(own_policy=False), "the policy belongs to another handle"),
    (dict(sampled=True), "sampling needs a Gaussian policy (salp_robot_policy_create_gaussian)"),
    (dict(max_steps=-1), "dt is too small (more than 2^24 Euler steps per cycle)"),
])
def test_refusals(kwargs, text):
    assert re_.check_evaluate(**{"max_steps": STEPS, "horizon": 4, **kwargs}) == (INVALID, text)


def test_a_short_message_buffer_is_not_overrun():
    rc, msg = re_.check_evaluate(STEPS, 0, msg_size=8)
    assert rc == INVALID and msg == "horizon"


def test_prototype_table_names_exactly_what_the_library_exports():
    path = native_lib.make("libsalp_robot_evaluate_host.so")
    r = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in r.stdout.splitlines() if line.split()[-1].startswith("salp_")}
    assert exported == set(re_.PROTOTYPES)
