"""CPU-only checks of mt_rollout_actor_critic's host side: the symbol is exported and prototyped, the ctypes mirror has the C
struct's layout (the nested mt_policy included), and what the host can refuse without a handle -- NULL, a wrong struct_size
in the outer struct or in the nested one, a critic's shape or scale, reserved, an output that needs a critic, a call that
asks for nothing new -- is refused before a device is touched.  What needs the handle (the ld's, the aliasing rules, sigma
against D, the LDS bound) is refused in tests/test_gpu_actor_critic_rollout.py."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("struct_size", "critic_layers", "policy", "critic_width", "critic_hidden_act", "critic_out_act", "critic_weight",
          "critic_bias", "critic_out_scale", "pad_", "logp_log", "logp_ld", "value_log", "value_ld", "last_value_out", "reserved")
POLICY_FIELDS = ("struct_size", "n_steps", "n_layers", "width", "hidden_act", "out_act", "draw", "weight", "bias", "out_scale",
                 "lo", "hi", "sigma", "flags", "action_log", "act_ld", "obs_log", "obs_ld", "reward_log", "done_log", "log_ld",
                 "return_out", "seed", "reserved")


@pytest.fixture(scope="module")
def lib():
    from manytor_amd import build, _lib
    build.build_library()            # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_call_is_exported_and_prototyped(lib):
    from manytor_amd import _lib
    assert hasattr(lib, "mt_rollout_actor_critic")
    res, args = _lib.PROTOTYPES["mt_rollout_actor_critic"]
    assert res is ctypes.c_int and args == [_lib._HANDLE, ctypes.POINTER(_lib.MtActorCritic)]
    assert lib.mt_version() >= 500


def test_ctypes_struct_matches_c_layout(lib, tmp_path):
    from manytor_amd import _lib
    items = ["sizeof(struct mt_actor_critic)"] + [f"offsetof(struct mt_actor_critic,{f})" for f in FIELDS]
    items += ["sizeof(struct mt_policy)"] + [f"offsetof(struct mt_actor_critic,policy.{f})" for f in POLICY_FIELDS]
    items += ["(size_t)MT_ACTOR_CRITIC_MAX_LDS"]
    src = tmp_path / "ac_sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "manytor_hip.h"\n'
                   f'int main(void){{printf("{" ".join(["%zu"] * len(items))}\\n", {", ".join(items)});return 0;}}\n')
    exe = tmp_path / "ac_sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S, P = _lib.MtActorCritic, _lib.MtPolicy
    assert [name for name, _ in S._fields_] == list(FIELDS)
    assert [name for name, _ in P._fields_] == list(POLICY_FIELDS)
    assert c == ([ctypes.sizeof(S)] + [getattr(S, f).offset for f in FIELDS]
                 + [ctypes.sizeof(P)] + [S.policy.offset + getattr(P, f).offset for f in POLICY_FIELDS]
                 + [_lib.ACTOR_CRITIC_MAX_LDS])


def _arg(_lib, critic=True):
    """Every scalar passes: with a NULL handle only the handle is missing."""
    s = _lib.MtActorCritic()
    s.struct_size = ctypes.sizeof(_lib.MtActorCritic)
    p = s.policy
    p.struct_size = ctypes.sizeof(_lib.MtPolicy)
    p.n_steps, p.n_layers, p.out_act, p.out_scale, p.lo, p.hi = 4, 1, _lib.ACT_TANH, 180.0, -180.0, 180.0
    p.sigma[:] = [1.0] * _lib.MT_MAX_DOF
    s.logp_log = 0x1000                                  # (an address nothing reads: no handle, no launch)
    if critic:
        s.critic_layers, s.critic_out_act, s.critic_out_scale = 2, _lib.ACT_IDENTITY, 1.0
        s.critic_hidden_act = _lib.ACT_TANH
        s.critic_width[0] = 8
        s.value_log = 0x2000
    return s


def test_null_arguments_are_invalid(lib):
    from manytor_amd import _lib
    for critic in (True, False):
        s = _arg(_lib, critic)
        assert lib.mt_rollout_actor_critic(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
        assert b"handle" in lib.mt_last_error(None)               # every scalar passed: only the handle is missing
    assert lib.mt_rollout_actor_critic(None, None) == _lib.MT_ERR_INVALID_ARG
    assert b"NULL" in lib.mt_last_error(None)


@pytest.mark.parametrize("nested", [False, True])
@pytest.mark.parametrize("delta", [-4, 4])
def test_bad_struct_size_is_invalid_and_names_the_field(lib, nested, delta):
    from manytor_amd import _lib
    s = _arg(_lib)
    if nested:
        s.policy.struct_size += delta
    else:
        s.struct_size += delta
    assert lib.mt_rollout_actor_critic(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    msg = lib.mt_last_error(None)
    assert (b"mt_actor_critic.policy.struct_size" if nested else b"mt_actor_critic.struct_size") in msg


@pytest.mark.parametrize("field, value, word", [
    ("critic_layers", -1, b"critic_layers"), ("critic_layers", 4, b"critic_layers"),
    ("critic_width", 0, b"critic_width[0]"), ("critic_width", 65, b"critic_width[0]"),
    ("critic_out_scale", float("nan"), b"critic_out_scale"), ("critic_out_scale", float("inf"), b"critic_out_scale"),
    ("critic_out_scale", float("-inf"), b"critic_out_scale"),
    ("critic_hidden_act", 0, b"critic_hidden_act"), ("critic_out_act", 2, b"critic_out_act"),
    ("reserved", 1, b"mt_actor_critic.reserved"), ("policy.reserved", 1, b"policy.reserved"),
    ("policy.sigma", 0.0, b"sigma[0]"), ("policy.sigma", float("nan"), b"sigma[0]"),
])
def test_scalars_are_screened_ahead_of_the_handle(lib, field, value, word):
    from manytor_amd import _lib
    s = _arg(_lib)
    if field == "critic_width":
        s.critic_width[0] = value
    elif field == "policy.sigma":
        s.policy.sigma[0] = value
    elif field == "policy.reserved":
        s.policy.reserved = value
    else:
        setattr(s, field, value)
    assert lib.mt_rollout_actor_critic(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert word in lib.mt_last_error(None)


def test_outputs_that_need_a_critic_and_a_call_that_asks_for_nothing(lib):
    from manytor_amd import _lib
    s = _arg(_lib, critic=False)
    s.value_log = 0x2000
    assert lib.mt_rollout_actor_critic(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"value_log needs a critic" in lib.mt_last_error(None)
    s = _arg(_lib, critic=False)
    s.last_value_out = 0x2000
    assert lib.mt_rollout_actor_critic(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"last_value_out needs a critic" in lib.mt_last_error(None)
    s = _arg(_lib, critic=False)
    s.logp_log = None
    assert lib.mt_rollout_actor_critic(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"mt_rollout_policy" in lib.mt_last_error(None)       # neither a critic nor logp_log: the message names the call to use
    # without logp_log a zero sigma is the deterministic policy, as in mt_rollout_policy: only the handle is missing
    s = _arg(_lib)
    s.logp_log = None
    s.policy.sigma[:] = [0.0] * _lib.MT_MAX_DOF
    assert lib.mt_rollout_actor_critic(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)
