"""CPU-only checks of mt_rollout_policy's host side: the symbol is exported and prototyped, the ctypes mirror of struct
mt_policy has the C struct's layout and constants, NULL arguments are refused before a device is touched, and the
reference the GPU test holds the kernel to (tests/policy_ref.py) is itself sound: the noise stream is a stream of its
own and bounded, and the fp32 restatement of the MLP stays within the action gate of the fp64 one."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cem_ref
import policy_ref
from oracle import manytor_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("struct_size", "n_steps", "n_layers", "width", "hidden_act", "out_act", "draw", "weight", "bias", "out_scale", "lo",
          "hi", "sigma", "flags", "action_log", "act_ld", "obs_log", "obs_ld", "reward_log", "done_log", "log_ld", "return_out",
          "seed", "reserved")
CONSTANTS = ("MT_POLICY_AUTO_RESET", "MT_POLICY_DRY_RUN", "MT_POLICY_SEE_POSE", "MT_POLICY_MAX_LAYERS", "MT_POLICY_MAX_WIDTH",
             "MT_ACT_IDENTITY", "MT_ACT_TANH", "MT_ACT_RELU")


@pytest.fixture(scope="module")
def lib():
    from manytor_amd import build, _lib
    build.build_library()            # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_rollout_policy_is_exported_and_prototyped(lib):
    from manytor_amd import _lib
    assert hasattr(lib, "mt_rollout_policy")
    res, args = _lib.PROTOTYPES["mt_rollout_policy"]
    assert res is ctypes.c_int and args == [_lib._HANDLE, ctypes.POINTER(_lib.MtPolicy)]
    assert lib.mt_version() >= 440


def test_ctypes_policy_matches_c_layout(lib, tmp_path):
    from manytor_amd import _lib
    src = tmp_path / "policy_sz.c"
    offsets = ", ".join(f"offsetof(struct mt_policy,{f})" for f in FIELDS)
    fmt = " ".join(["%zu"] * (len(FIELDS) + 1) + ["%d"] * len(CONSTANTS))
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "manytor_hip.h"\n'
        f'int main(void){{printf("{fmt}\\n", sizeof(struct mt_policy), {offsets}, '
        + ", ".join(f"(int){c}" for c in CONSTANTS) + ');return 0;}\n')
    exe = tmp_path / "policy_sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _lib.MtPolicy
    assert [name for name, _ in S._fields_] == list(FIELDS)
    mirror = [_lib.POLICY_AUTO_RESET, _lib.POLICY_DRY_RUN, _lib.POLICY_SEE_POSE, _lib.POLICY_MAX_LAYERS, _lib.POLICY_MAX_WIDTH,
              _lib.ACT_IDENTITY, _lib.ACT_TANH, _lib.ACT_RELU]
    assert c == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + mirror
    assert S.sigma.size == 4 * _lib.MT_MAX_DOF


def test_null_arguments_are_invalid(lib):
    from manytor_amd import _lib
    p = _lib.MtPolicy()
    p.struct_size = ctypes.sizeof(_lib.MtPolicy)
    assert lib.mt_rollout_policy(None, ctypes.byref(p)) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)
    assert lib.mt_rollout_policy(None, None) == _lib.MT_ERR_INVALID_ARG


# ---- the noise stream ---------------------------------------------------------------------------------------------
def test_policy_stream_is_not_the_plan_stream():
    env = np.arange(4096, dtype=np.uint64) + np.uint64(1 << 33)
    for D in (4, 7):
        z4 = policy_ref.policy_noise(0xABCDEF0123, env, 5, 3, D)
        z3 = cem_ref.plan_noise(0xABCDEF0123, env, 5, 1, 3, D)[0]      # candidate 0: the same counter but for the tag
        assert z4.shape == z3.shape == (3, D, env.size)
        assert np.mean(z4 == z3) < 0.02                                 # (z takes ~1000 values: chance equality is rare)
        assert abs(float(z4.mean())) < 0.02 and abs(float(z4.std()) - 1.0) < 0.02


def test_policy_noise_is_bounded():
    z = policy_ref.policy_noise(7, np.arange(20000, dtype=np.uint64), 0, 2, 8)
    assert float(np.abs(z).max()) <= cem_ref.Z_MAX
    assert float(np.abs(cem_ref.noise(np.array([0, 0xFFFFFFFF], dtype=np.uint32))).max()) <= cem_ref.Z_MAX
    # steps past the first continue the stream: t0 shifts it
    np.testing.assert_array_equal(policy_ref.policy_noise(7, np.arange(64, dtype=np.uint64), 0, 1, 8, t0=1)[0], z[1][:, :64])


# ---- the MLP reference ---------------------------------------------------------------------------------------------
# The GPU test's six shapes (tests/test_gpu_policy.py), observed at the zero pose with reference-style targets.
SHAPES = [
    ("ref", 7, (32, 32), "tanh", "tanh", False),
    ("ref", 1, (), "tanh", "tanh", False),
    ("ref", 32, (64, 64), "relu", "identity", True),
    ("dh7", 3, (17, 5), "tanh", "tanh", False),
    ("rt5", 3, (32,), "tanh", "tanh", True),
    ("ref", 2, (3, 1), "tanh", "tanh", False),
]


def _zero_pose_inputs(name, k, see_pose, n=300):
    import staged_populations as sp
    from manytor_amd.engine import DH7_TABLE, REF_DH_TABLE
    table, radius = {"ref": (REF_DH_TABLE, 51.3), "dh7": (DH7_TABLE, 92.6), "rt5": sp.fractional_offset_table()}[name]
    table = np.asarray(table, dtype=np.float64)
    dof = table.shape[0]
    rng = np.random.RandomState(k + dof)
    v = rng.randn(n, k, 3)
    pts = v / np.linalg.norm(v, axis=-1, keepdims=True) * radius * rng.uniform(0.2, 1.0, (n, k, 1)) ** (1 / 3)
    pts[..., 2] = np.abs(pts[..., 2])
    goals = np.zeros((n, dof))
    elbow = mo.batch_joints_coordinates(goals, table)[:, -2]
    x = mo.observe(elbow, pts, np.ones((n, k), dtype=bool)).T            # (3K, n)
    if see_pose:
        x = np.concatenate([x, goals.T])
    return x.astype(np.float32), dof


@pytest.mark.parametrize("name,k,widths,hidden,out,see_pose", SHAPES)
def test_fp32_mlp_stays_within_the_action_gate_of_fp64(name, k, widths, hidden, out, see_pose):
    x, dof = _zero_pose_inputs(name, k, see_pose)
    layers = policy_ref.make_weights(1234 + k, x.shape[0], widths, dof)
    pre = []
    a64 = policy_ref.mlp(x, layers, hidden, out, 180.0, np.float64, pre)
    a32 = policy_ref.mlp(x, layers, hidden, out, 180.0, np.float32)
    err = float(np.abs(a32.astype(np.float64) - a64).max())
    print(f"{name} K={k} widths={widths}: fp32 vs fp64 {err:.3g} deg; hidden pre-activation std "
          + ", ".join(f"{float(y.std()):.2f}" for y in pre))
    assert err <= policy_ref.ACTION_TOL_DEG
    assert np.all(np.isfinite(a64))


def test_clamp_hands_unusable_values_on():
    a = np.array([np.nan, np.inf, -40000.0, 32768.0, 200.0, -200.0, 12.5], dtype=np.float32)
    got = policy_ref.clamp(a, -180.0, 180.0)
    np.testing.assert_array_equal(got[3:], np.array([180.0, 180.0, -180.0, 12.5], dtype=np.float32))
    assert np.isnan(got[0]) and np.isinf(got[1]) and got[2] == np.float32(-40000.0)
