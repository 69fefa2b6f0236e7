"""CPU-only checks of mt_policy_grad / mt_reward_to_go's host side: the symbols are exported and prototyped, the ctypes
mirrors have the C structs' layout, and what the host can refuse without a handle -- NULL, a wrong struct_size, a sigma that is
not positive, a scale that is not finite -- is refused before a device is touched (what needs the handle's shape, the
workspace size and the aliasing rules, is refused in tests/test_gpu_policy_grad.py); and the restatement the GPU test holds
the kernels to (tests/pg_ref.py) is itself sound."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import pg_ref
import policy_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {
    "mt_policy_grad": ("MtPolicyGrad", ("struct_size", "n_steps", "n_layers", "width", "hidden_act", "out_act", "weight", "bias",
                                        "out_scale", "sigma", "flags", "obs", "obs_ld", "action", "act_ld", "coef", "coef_ld",
                                        "scale", "grad_out", "loss_out", "workspace", "workspace_bytes", "reserved")),
    "mt_reward_to_go": ("MtRewardToGo", ("struct_size", "n_steps", "reward_log", "done_log", "log_ld", "gamma", "baseline", "out",
                                         "out_ld", "flags", "reserved")),
}
ENTRY = {"mt_policy_grad": "MtPolicyGrad", "mt_reward_to_go": "MtRewardToGo"}


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
    assert hasattr(lib, "mt_policy_grad_workspace")
    assert _lib.PROTOTYPES["mt_policy_grad_workspace"][0] is ctypes.c_size_t
    assert lib.mt_version() >= 460


def test_ctypes_structs_match_c_layout(lib, tmp_path):
    from manytor_amd import _lib
    items, fmt = [], []
    for cname, (_, fields) in STRUCTS.items():
        items.append(f"sizeof(struct {cname})")
        items += [f"offsetof(struct {cname},{f})" for f in fields]
        fmt += ["%zu"] * (len(fields) + 1)
    items.append("(size_t)MT_RTG_MASK_AFTER_DONE")
    fmt.append("%zu")
    src = tmp_path / "pg_sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "manytor_hip.h"\n'
                   f'int main(void){{printf("{" ".join(fmt)}\\n", {", ".join(items)});return 0;}}\n')
    exe = tmp_path / "pg_sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, (pyname, fields) in STRUCTS.items():
        S = getattr(_lib, pyname)
        assert [name for name, _ in S._fields_] == list(fields)
        want += [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields]
    want.append(_lib.RTG_MASK_AFTER_DONE)
    assert c == want


def _grad_arg(_lib):
    s = _lib.MtPolicyGrad()
    s.struct_size = ctypes.sizeof(_lib.MtPolicyGrad)
    s.n_layers, s.out_act, s.out_scale, s.scale = 1, _lib.ACT_TANH, 180.0, 1.0
    s.sigma[:] = [1.0] * _lib.MT_MAX_DOF
    return s


def _rtg_arg(_lib):
    s = _lib.MtRewardToGo()
    s.struct_size = ctypes.sizeof(_lib.MtRewardToGo)
    s.gamma = 1.0
    return s


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_null_arguments_are_invalid(lib, name):
    from manytor_amd import _lib
    s = _grad_arg(_lib) if name == "mt_policy_grad" else _rtg_arg(_lib)
    fn = getattr(lib, name)
    assert fn(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)
    assert fn(None, None) == _lib.MT_ERR_INVALID_ARG
    assert lib.mt_policy_grad_workspace(None, 1, None, 0, 3) == 0


@pytest.mark.parametrize("name", sorted(ENTRY))
@pytest.mark.parametrize("delta", [-8, 8, None])
def test_bad_struct_size_is_invalid(lib, name, delta):
    from manytor_amd import _lib
    S = getattr(_lib, ENTRY[name])
    s = S()
    s.struct_size = 0 if delta is None else ctypes.sizeof(S) + delta
    assert getattr(lib, name)(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"struct_size" in lib.mt_last_error(None)


@pytest.mark.parametrize("field, value, word", [
    ("sigma", 0.0, b"sigma"), ("sigma", -1.0, b"sigma"), ("sigma", float("nan"), b"sigma"), ("sigma", float("inf"), b"sigma"),
    ("scale", float("nan"), b"scale"), ("scale", float("inf"), b"scale"), ("out_scale", float("-inf"), b"out_scale"),
    ("n_layers", 4, b"n_layers"), ("n_steps", -1, b"n_steps"), ("flags", 1, b"flags"), ("reserved", 1, b"reserved"),
])
def test_policy_grad_scalars_are_screened_ahead_of_the_handle(lib, field, value, word):
    from manytor_amd import _lib
    s = _grad_arg(_lib)
    if field == "sigma":
        s.sigma[0] = value
    else:
        setattr(s, field, value)
    assert lib.mt_policy_grad(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert word in lib.mt_last_error(None)


@pytest.mark.parametrize("field, value", [("gamma", 1.5), ("gamma", -0.1), ("gamma", float("nan")), ("baseline", float("inf")),
                                          ("flags", 2), ("reserved", 1)])
def test_reward_to_go_scalars_are_screened_ahead_of_the_handle(lib, field, value):
    from manytor_amd import _lib
    s = _rtg_arg(_lib)
    setattr(s, field, value)
    assert lib.mt_reward_to_go(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert field.encode() in lib.mt_last_error(None)


# ---- pg_ref's own soundness ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths, hidden, out", [((), "tanh", "tanh"), ((3,), "tanh", "identity"), ((4, 3), "tanh", "tanh")])
def test_fp64_gradient_agrees_with_a_central_difference_of_its_own_loss(widths, hidden, out):
    rng = np.random.RandomState(7)
    n_in, dof, S = 5, 2, 9
    layers = policy_ref.make_weights(3, n_in, widths, dof)
    layers = [(w * np.float32(20), b) for w, b in layers]            # out of the linear range of the first layer
    x = rng.randn(n_in, S).astype(np.float32)
    a = (40 * rng.randn(dof, S)).astype(np.float32)
    c = rng.randn(S).astype(np.float32)
    c[2] = 0
    a[1, 4] = np.nan                                                 # skipped, not poisoned
    sigma = np.array([3.0, 7.0], dtype=np.float32)
    grad, abs_sum, loss = pg_ref.policy_grad(layers, x, a, c, sigma, hidden, out, 180.0)
    assert np.isfinite(grad).all() and np.isfinite(loss) and (abs_sum >= np.abs(grad) * (1 - 1e-12)).all()
    shapes = [w.shape for w, _ in layers]
    theta = pg_ref.flatten(layers).astype(np.float64)
    fd = np.empty_like(theta)
    for i in range(theta.size):
        step = 1e-6 * max(1.0, abs(theta[i]))
        vals = []
        for sgn in (1, -1):
            th = theta.copy()
            th[i] += sgn * step
            lay = [(w.astype(np.float64), b.astype(np.float64)) for w, b in pg_ref.unflatten(th, shapes)]
            vals.append(_loss64(lay, x, a, c, sigma, hidden, out, 180.0))
        fd[i] = (vals[0] - vals[1]) / (2 * step)
    np.testing.assert_allclose(grad, fd, rtol=2e-5, atol=2e-5 * float(np.abs(grad).max()))


def _loss64(layers, x, a, c, sigma, hidden, out, out_scale):
    """sum_s c_s logp_s in fp64 for fp64 weights, written out on its own (pg_ref rounds its weights to fp32)."""
    keep = pg_ref.usable_samples(a, c)
    h = x.astype(np.float64)[:, keep]
    for l, (w, b) in enumerate(layers):
        y = w @ h + b[:, None]
        act = out if l == len(layers) - 1 else hidden
        h = np.tanh(y) if act == "tanh" else np.maximum(y, 0) if act == "relu" else y
    e = (a.astype(np.float64)[:, keep] - out_scale * h) / sigma.astype(np.float64)[:, None]
    return float((c.astype(np.float64)[keep] * (-0.5 * (e * e).sum(axis=0))).sum())


def test_fp32_restatement_is_close_to_fp64():
    rng = np.random.RandomState(11)
    n_in, dof, S = 21, 4, 512
    layers = policy_ref.make_weights(5, n_in, (33, 64), dof)
    x = (30 * rng.randn(n_in, S)).astype(np.float32)
    a = (60 * rng.randn(dof, S)).astype(np.float32)
    c = rng.randn(S).astype(np.float32)
    g64, abs_sum, _ = pg_ref.policy_grad(layers, x, a, c, np.full(dof, 5.0), "tanh", "tanh", 180.0)
    g32, _, _ = pg_ref.policy_grad(layers, x, a, c, np.full(dof, 5.0), "tanh", "tanh", 180.0, dtype=np.float32)
    assert g32.dtype == np.float32
    ratio = np.abs(g32 - g64)[abs_sum > 0] / abs_sum[abs_sum > 0]
    assert ratio.max() < 1e-5


def _round_f32(fr):
    """The fp32 nearest to a Fraction, ties to even."""
    v = np.float32(float(fr))
    cands = {float(v), float(np.nextafter(v, np.float32(np.inf))), float(np.nextafter(v, np.float32(-np.inf)))}
    best = min(cands, key=lambda q: (abs(Fraction(q) - fr), int(np.float32(q).view(np.uint32)) & 1))
    return np.float32(best)


@pytest.mark.parametrize("gamma", [1.0, 0.5, 0.99])
@pytest.mark.parametrize("mask", [False, True])
def test_reward_to_go_agrees_with_a_plain_loop(gamma, mask):
    rng = np.random.RandomState(5)
    T, n = 9, 40
    reward = rng.randint(-1, 2, size=(T, n)).astype(np.int8)
    done = (rng.rand(T, n) < 0.2).astype(np.uint8)
    done[:, 0] = 0
    done[0, 1] = 1
    done[:, 2] = 0
    done[T - 1, 2] = 1
    base = np.float32(0.375)
    got = pg_ref.reward_to_go(reward, done, gamma, base, mask)
    assert got.dtype == np.float32
    g = Fraction(float(np.float32(gamma)))
    for i in range(n):
        R, first = np.float32(0), T
        for t in range(T):
            if done[t, i]:
                first = t
                break
        for t in range(T - 1, -1, -1):
            if mask and t > first:
                assert got[t, i] == 0
                continue
            nxt = Fraction(0) if done[t, i] else Fraction(float(R))
            R = _round_f32(g * nxt + int(reward[t, i]))
            assert got[t, i] == np.float32(R - base), (t, i)
    if gamma == 1.0 and not mask:                                # (masked entries are 0, not -baseline)
        np.testing.assert_array_equal(got + base, np.round(got + base))


def test_fma32_rounds_once():
    a = np.float32(1 + 2.0 ** -12)
    # a * a = 1 + 2^-11 + 2^-24; with c = -(1 + 2^-11) the fused result is 2^-24, a rounded product would give 0
    c = -np.float32(1 + 2.0 ** -11)
    assert pg_ref.fma32(a, a, c) == np.float32(2.0 ** -24)
    # a double-rounding case: 2^-24 (1 + 2^-23) (1 - 2^-23) = 2^-24 - 2^-70, so with c = 1 + 2^-23 the exact sum lies just BELOW
    # the fp32 midpoint; a sum rounded to fp64 first lands on the midpoint and then goes up, to the even neighbour
    x, y, c = np.float32(2.0 ** -24 * (1 + 2.0 ** -23)), np.float32(1 - 2.0 ** -23), np.float32(1 + 2.0 ** -23)
    assert np.float32(np.float64(x) * np.float64(y) + np.float64(c)) == np.float32(1 + 2.0 ** -22)
    assert pg_ref.fma32(x, y, c) == c
