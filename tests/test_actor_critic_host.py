"""CPU-only checks of mt_policy_eval / mt_gae / mt_value_grad's host side: the symbols are exported and prototyped, the
ctypes mirrors have the C structs' layout, and what the host can refuse without a handle is refused before a device is
touched (what needs the handle's shape is refused in the GPU tests); and the restatement the GPU tests hold the kernels to
(tests/ac_ref.py) is itself sound."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ac_ref
import pg_ref
import policy_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_NET = ("struct_size", "n_steps", "n_layers", "width", "hidden_act", "out_act", "weight", "bias", "out_scale", "flags", "obs", "obs_ld")
STRUCTS = {
    "mt_policy_eval": ("MtPolicyEval", _NET + ("n_out", "mean_out", "mean_ld", "action", "act_ld", "sigma", "logp_out", "logp_ld",
                                               "reserved")),
    "mt_gae": ("MtGae", ("struct_size", "n_steps", "reward_log", "done_log", "log_ld", "value", "value_ld", "last_value", "gamma",
                         "lambda", "adv_out", "adv_ld", "ret_out", "ret_ld", "weight_out", "weight_ld", "flags", "reserved")),
    "mt_value_grad": ("MtValueGrad", _NET + ("target", "target_ld", "coef", "coef_ld", "scale", "grad_out", "loss_out", "workspace",
                                             "workspace_bytes", "reserved")),
}
ENTRY = {name: py for name, (py, _) in STRUCTS.items()}


def py_field(name):
    return name + "_" if name == "lambda" else name              # (a Python keyword)


@pytest.fixture(scope="module")
def lib():
    from manytor_amd import build, _lib
    build.build_library()            # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_calls_are_exported_and_prototyped(lib):
    from manytor_amd import _lib
    for name, struct in ENTRY.items():
        assert hasattr(lib, name)
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and args == [_lib._HANDLE, ctypes.POINTER(getattr(_lib, struct))]
    assert hasattr(lib, "mt_value_grad_workspace")
    assert _lib.PROTOTYPES["mt_value_grad_workspace"] == _lib.PROTOTYPES["mt_policy_grad_workspace"]
    assert lib.mt_version() >= 470


def test_ctypes_structs_match_c_layout(lib, tmp_path):
    from manytor_amd import _lib
    items, fmt = [], []
    for cname, (_, fields) in STRUCTS.items():
        items.append(f"sizeof(struct {cname})")
        items += [f"offsetof(struct {cname},{f})" for f in fields]
        fmt += ["%zu"] * (len(fields) + 1)
    items.append("(size_t)MT_GAE_MASK_AFTER_DONE")
    fmt.append("%zu")
    src = tmp_path / "ac_sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "manytor_hip.h"\n'
                   f'int main(void){{printf("{" ".join(fmt)}\\n", {", ".join(items)});return 0;}}\n')
    exe = tmp_path / "ac_sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, (pyname, fields) in STRUCTS.items():
        S = getattr(_lib, pyname)
        assert [name for name, _ in S._fields_] == [py_field(f) for f in fields]
        want += [ctypes.sizeof(S)] + [getattr(S, py_field(f)).offset for f in fields]
    want.append(_lib.GAE_MASK_AFTER_DONE)
    assert c == want


def _arg(_lib, name):
    s = getattr(_lib, ENTRY[name])()
    s.struct_size = ctypes.sizeof(s)
    if name == "mt_gae":
        s.gamma, s.lambda_ = 0.99, 0.95
        return s
    s.n_layers, s.out_act, s.out_scale = 1, _lib.ACT_IDENTITY, 1.0
    if name == "mt_value_grad":
        s.scale = 1.0
    else:
        s.sigma[:] = [1.0] * _lib.MT_MAX_DOF
        s.mean_out = 4096                                        # (never dereferenced: the handle is NULL)
    return s


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_null_arguments_are_invalid(lib, name):
    from manytor_amd import _lib
    fn = getattr(lib, name)
    assert fn(None, ctypes.byref(_arg(_lib, name))) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)
    assert fn(None, None) == _lib.MT_ERR_INVALID_ARG
    assert lib.mt_value_grad_workspace(None, 1, None, 0, 3) == 0


@pytest.mark.parametrize("name", sorted(ENTRY))
@pytest.mark.parametrize("delta", [-8, 8, None])
def test_bad_struct_size_is_invalid(lib, name, delta):
    from manytor_amd import _lib
    S = getattr(_lib, ENTRY[name])
    s = S()
    s.struct_size = 0 if delta is None else ctypes.sizeof(S) + delta
    assert getattr(lib, name)(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"struct_size" in lib.mt_last_error(None)


@pytest.mark.parametrize("name, field, value, word", [
    ("mt_policy_eval", "out_scale", float("nan"), b"out_scale"), ("mt_policy_eval", "n_layers", 0, b"n_layers"),
    ("mt_policy_eval", "n_out", 9, b"n_out"), ("mt_policy_eval", "n_out", -1, b"n_out"), ("mt_policy_eval", "flags", 2, b"flags"),
    ("mt_policy_eval", "mean_out", None, b"both NULL"), ("mt_policy_eval", "logp_out", 4096, b"needs action"),
    ("mt_policy_eval", "reserved", 1, b"reserved"), ("mt_policy_eval", "n_steps", 65536, b"n_steps"),
    ("mt_gae", "gamma", 1.5, b"gamma"), ("mt_gae", "gamma", float("nan"), b"gamma"), ("mt_gae", "lambda_", -0.25, b"lambda"),
    ("mt_gae", "lambda_", float("inf"), b"lambda"), ("mt_gae", "flags", 2, b"flags"), ("mt_gae", "reserved", 1, b"reserved"),
    ("mt_value_grad", "scale", float("inf"), b"scale"), ("mt_value_grad", "out_scale", float("nan"), b"out_scale"),
    ("mt_value_grad", "out_act", 2, b"out_act"), ("mt_value_grad", "n_layers", 4, b"n_layers"),
    ("mt_value_grad", "reserved", 1, b"reserved"),
])
def test_scalars_are_screened_ahead_of_the_handle(lib, name, field, value, word):
    from manytor_amd import _lib
    s = _arg(_lib, name)
    setattr(s, field, value)
    assert getattr(lib, name)(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert word in lib.mt_last_error(None)


@pytest.mark.parametrize("sigma", [0.0, -1.0, float("nan"), float("inf")])
def test_policy_eval_screens_sigma_only_when_logp_reads_it(lib, sigma):
    from manytor_amd import _lib
    s = _arg(_lib, "mt_policy_eval")
    s.sigma[0] = sigma
    assert lib.mt_policy_eval(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)                  # the mean alone: sigma is not read
    s.logp_out, s.action = 4096, 8192
    assert lib.mt_policy_eval(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"sigma[0]" in lib.mt_last_error(None)


# ---- ac_ref's own soundness ---------------------------------------------------------------------------------------------
def _logs(T, n=300, seed=5):
    rng = np.random.RandomState(seed + T)
    reward = rng.randint(-128, 128, size=(T, n)).astype(np.int8)
    done = (rng.rand(T, n) < 0.2).astype(np.uint8)
    value = (10 * rng.randn(T, n)).astype(np.float32)
    last = (10 * rng.randn(n)).astype(np.float32)
    return reward, done, value, last


@pytest.mark.parametrize("T", [1, 3, 7])
@pytest.mark.parametrize("gamma", [1.0, 0.99])
@pytest.mark.parametrize("mask", [False, True])
def test_gae_with_lambda_one_and_no_critic_is_the_reward_to_go(T, gamma, mask):
    reward, done, value, _ = _logs(T)
    adv, ret, weight = ac_ref.gae(reward, done, np.zeros_like(value), None, gamma, 1.0, mask)
    want = pg_ref.reward_to_go(reward, done, gamma, 0.0, mask)
    assert adv.dtype == np.float32
    np.testing.assert_array_equal(adv.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(ret, adv)


@pytest.mark.parametrize("T", [1, 3, 7])
@pytest.mark.parametrize("gamma", [1.0, 0.99])
def test_gae_with_lambda_zero_is_the_td_residual(T, gamma):
    reward, done, value, last = _logs(T)
    adv, ret, weight = ac_ref.gae(reward, done, value, last, gamma, 0.0, False)
    nxt = np.concatenate([value[1:], last[None]])
    nv = np.where(done != 0, np.float32(0), nxt)
    want = (pg_ref.fma32(np.float32(gamma), nv, reward.astype(np.float32)) - value).astype(np.float32)
    np.testing.assert_array_equal(adv, want)
    np.testing.assert_array_equal(ret, (want + value).astype(np.float32))
    assert (weight == 1).all()


@pytest.mark.parametrize("T", [1, 3, 7])
def test_masked_gae_writes_zeros_behind_the_first_done(T):
    reward, done, value, last = _logs(T)
    done[:, 0] = 0
    done[0, 1] = 1
    plain = ac_ref.gae(reward, done, value, last, 0.99, 0.95, False)
    poisoned = np.array(value)
    behind = np.zeros(done.shape, dtype=bool)
    behind[1:] = np.cumsum(done, axis=0)[:-1] > 0
    poisoned[behind] = np.nan                                    # a masked step's value is never looked at
    adv, ret, weight = ac_ref.gae(reward, done, poisoned, last, 0.99, 0.95, True)
    for got, ref in zip((adv, ret, weight), plain):
        assert (got[behind] == 0).all()
        # up to and at the first done that done cuts the recurrence anyway: the unmasked numbers
        np.testing.assert_array_equal(got[~behind], ref[~behind])
    np.testing.assert_array_equal(weight, (~behind).astype(np.float32))
    assert (~behind).any() and (T == 1 or behind.any())
    assert np.isfinite(adv).all() and np.isfinite(ret).all()


def test_logp_is_the_stated_sequence():
    rng = np.random.RandomState(3)
    mean = (90 * rng.randn(2, 4, 50)).astype(np.float32)
    a = (90 * rng.randn(2, 4, 50)).astype(np.float32)
    sigma = np.array([3.0, 7.0, 20.0, 0.5], dtype=np.float32)
    a[0, 1, 4], a[1, 3, 7], a[1, 0, 9], a[0, 2, 11] = np.nan, np.inf, 40000.0, -32768.0   # the last one is usable
    got = ac_ref.logp(mean, a, sigma)
    assert got.dtype == np.float32 and got.shape == (2, 50)
    assert got[0, 4] == 0 and got[1, 7] == 0 and got[1, 9] == 0 and got[0, 11] < 0
    e = a.astype(np.float64) - mean
    want = -0.5 * ((e / sigma[:, None].astype(np.float64)) ** 2).sum(axis=1)
    ok = np.isfinite(want) & (got != 0)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-6)
    inv_var = (1.0 / sigma.astype(np.float64) ** 2).astype(np.float32)
    lp = np.float32(0)
    for j in range(4):                                           # one sample, by hand
        ej = np.float32(a[1, j, 20] - mean[1, j, 20])
        lp = pg_ref.fma32(ej, np.float32(ej * inv_var[j]), lp)
    assert got[1, 20] == np.float32(-0.5) * lp


def _value_loss64(layers, x, target, c, hidden, out, out_scale):
    """sum_s c_s (-1/2 (R_s - V_s)^2) in fp64 for fp64 weights, written out on its own (pg_ref rounds its weights to fp32)."""
    keep = pg_ref.usable_samples(target[None], c)
    h = x.astype(np.float64)[:, keep]
    for l, (w, b) in enumerate(layers):
        y = w @ h + b[:, None]
        act = out if l == len(layers) - 1 else hidden
        h = np.tanh(y) if act == "tanh" else np.maximum(y, 0) if act == "relu" else y
    e = target.astype(np.float64)[keep] - out_scale * h[0]
    return float((c.astype(np.float64)[keep] * (-0.5 * e * e)).sum())


@pytest.mark.parametrize("out, out_scale", [("identity", 1.0), ("tanh", 5.0)])
def test_fp64_value_gradient_agrees_with_a_central_difference_of_its_own_loss(out, out_scale):
    rng = np.random.RandomState(7)
    n_in, S = 6, 50
    layers = policy_ref.make_weights(3, n_in, (5,), 1)
    layers = [(w * np.float32(20) if l == 0 else w, b) for l, (w, b) in enumerate(layers)]
    x = rng.randn(n_in, S).astype(np.float32)
    target = (2 * rng.randn(S)).astype(np.float32)
    c = rng.rand(S).astype(np.float32)
    c[2] = 0
    target[4] = np.nan                                           # skipped, not poisoned
    grad, abs_sum, loss = ac_ref.value_grad(layers, x, target, c, "tanh", out, out_scale)
    assert np.isfinite(grad).all() and np.isfinite(loss) and (abs_sum >= np.abs(grad) * (1 - 1e-12)).all()
    assert abs(loss - _value_loss64([(w.astype(np.float64), b.astype(np.float64)) for w, b in layers], x, target, c, "tanh", out,
                                    out_scale)) <= 1e-12 * abs(loss)
    shapes = [w.shape for w, _ in layers]
    theta = pg_ref.flatten(layers).astype(np.float64)
    fd = np.empty_like(theta)
    for i in range(theta.size):
        step = 1e-5 * max(1.0, abs(theta[i]))
        vals = []
        for sgn in (1, -1):
            th = theta.copy()
            th[i] += sgn * step
            vals.append(_value_loss64(pg_ref.unflatten(th, shapes), x, target, c, "tanh", out, out_scale))
        fd[i] = (vals[0] - vals[1]) / (2 * step)
    assert np.abs(grad - fd).max() <= 1e-6 * np.abs(grad).max()


def test_value_constants_are_consistent():
    """The gate of the one-output head is 4 x what was measured on the GPU and at most 16 x the plain fp32 restatement."""
    assert ac_ref.VALUE_MEASURED > 0 and ac_ref.VALUE_REF32_MEASURED > 0
    assert ac_ref.VALUE_TOL == 4.0 * ac_ref.VALUE_MEASURED
    assert ac_ref.VALUE_TOL <= 16.0 * ac_ref.VALUE_REF32_MEASURED
