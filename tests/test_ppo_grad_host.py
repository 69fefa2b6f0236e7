"""CPU-only checks of mt_ppo_grad's host side: the symbols are exported and prototyped, the ctypes mirror has the C struct's
layout, and what the host can refuse without a handle -- NULL, a wrong struct_size, a clip outside {0} u (0, 1), a shift or a
scale that is not finite, a sigma that is not positive, flags, reserved -- is refused before a device is touched (what needs
the handle's shape, the workspace size and the aliasing rules, is refused in tests/test_gpu_ppo_grad.py); and the restatement
the GPU test holds the kernels to (tests/ppo_ref.py) is itself sound: its gradients in theta and in log sigma are the
central differences of the clipped surrogate written out on its own, from the full Gaussian density."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import pg_ref
import policy_ref
import ppo_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("struct_size", "n_steps", "n_layers", "width", "hidden_act", "out_act", "weight", "bias", "out_scale", "sigma", "flags",
          "obs", "obs_ld", "action", "act_ld", "adv", "adv_ld", "old_logp", "old_ld", "sample_weight", "weight_ld", "clip",
          "log_ratio_shift", "scale", "grad_out", "loss_out", "ratio_out", "ratio_ld", "coef_out", "coef_ld", "sigma_grad_out",
          "kl_out", "count_out", "workspace", "workspace_bytes", "reserved")


@pytest.fixture(scope="module")
def lib():
    from manytor_amd import build, _lib
    build.build_library()            # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_calls_are_exported_and_prototyped(lib):
    from manytor_amd import _lib
    assert hasattr(lib, "mt_ppo_grad") and hasattr(lib, "mt_ppo_grad_workspace")
    res, args = _lib.PROTOTYPES["mt_ppo_grad"]
    assert res is ctypes.c_int and args == [_lib._HANDLE, ctypes.POINTER(_lib.MtPpoGrad)]
    assert _lib.PROTOTYPES["mt_ppo_grad_workspace"] == _lib.PROTOTYPES["mt_policy_grad_workspace"]
    assert lib.mt_version() >= 490


def test_ctypes_struct_matches_c_layout(lib, tmp_path):
    from manytor_amd import _lib
    items = ["sizeof(struct mt_ppo_grad)"] + [f"offsetof(struct mt_ppo_grad,{f})" for f in FIELDS]
    items += ["(size_t)MT_PPO_EXTRA_WORDS", "(size_t)MT_PPO_MAX_LOG_RATIO"]
    src = tmp_path / "ppo_sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "manytor_hip.h"\n'
                   f'int main(void){{printf("{" ".join(["%zu"] * len(items))}\\n", {", ".join(items)});return 0;}}\n')
    exe = tmp_path / "ppo_sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _lib.MtPpoGrad
    assert [name for name, _ in S._fields_] == list(FIELDS)
    assert c == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + [_lib.PPO_EXTRA_WORDS, int(_lib.PPO_MAX_LOG_RATIO)]
    assert ppo_ref.MAX_LOG_RATIO == _lib.PPO_MAX_LOG_RATIO


def _arg(_lib):
    s = _lib.MtPpoGrad()
    s.struct_size = ctypes.sizeof(_lib.MtPpoGrad)
    s.n_layers, s.out_act, s.out_scale, s.scale, s.clip = 1, _lib.ACT_TANH, 180.0, 1.0, 0.2
    s.sigma[:] = [1.0] * _lib.MT_MAX_DOF
    return s


def test_null_arguments_are_invalid(lib):
    from manytor_amd import _lib
    s = _arg(_lib)
    assert lib.mt_ppo_grad(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)                   # every scalar passed: only the handle is missing
    s.clip = 0.0                                                  # no clipping is a legal value
    assert lib.mt_ppo_grad(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)
    assert lib.mt_ppo_grad(None, None) == _lib.MT_ERR_INVALID_ARG
    assert lib.mt_ppo_grad_workspace(None, 1, None, 0, 3) == 0


@pytest.mark.parametrize("delta", [-8, 8, None])
def test_bad_struct_size_is_invalid(lib, delta):
    from manytor_amd import _lib
    s = _lib.MtPpoGrad()
    s.struct_size = 0 if delta is None else ctypes.sizeof(_lib.MtPpoGrad) + delta
    assert lib.mt_ppo_grad(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"struct_size" in lib.mt_last_error(None)


@pytest.mark.parametrize("field, value, word", [
    ("clip", -0.1, b"clip"), ("clip", 1.0, b"clip"), ("clip", float("nan"), b"clip"), ("clip", float("inf"), b"clip"),
    ("log_ratio_shift", float("nan"), b"log_ratio_shift"), ("log_ratio_shift", float("inf"), b"log_ratio_shift"),
    ("log_ratio_shift", float("-inf"), b"log_ratio_shift"),
    ("scale", float("nan"), b"scale"), ("scale", float("inf"), b"scale"), ("out_scale", float("-inf"), b"out_scale"),
    ("sigma", 0.0, b"sigma"), ("sigma", -1.0, b"sigma"), ("sigma", float("nan"), b"sigma"), ("sigma", float("inf"), b"sigma"),
    ("n_layers", 4, b"n_layers"), ("n_steps", -1, b"n_steps"), ("reserved", 1, b"reserved"),
    ("flags", 1, b"flags"), ("flags", 2, b"flags"), ("flags", 4 | 8, b"flags"),
])
def test_scalars_are_screened_ahead_of_the_handle(lib, field, value, word):
    from manytor_amd import _lib
    s = _arg(_lib)
    if field == "sigma":
        s.sigma[0] = value
    else:
        setattr(s, field, value)
    assert lib.mt_ppo_grad(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert word in lib.mt_last_error(None)


def test_see_pose_alone_passes_the_flag_screen(lib):
    from manytor_amd import _lib
    s = _arg(_lib)
    s.flags = _lib.POLICY_SEE_POSE
    assert lib.mt_ppo_grad(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)


# ---- ppo_ref's own soundness --------------------------------------------------------------------------------------------
CLIP = 0.2


def _surrogate64(layers, log_sigma, x, a, adv, w, old_full, hidden, out, out_scale):
    """sum_s w_s min(ratio adv, clamp(ratio, 1 - clip, 1 + clip) adv) in fp64 for fp64 weights and log sigma, written out on
    its own: ratio = p(a | x) / p_old from the FULL Gaussian log-density, -1/2 sum ((a - mu) / sigma)^2 - sum log sigma."""
    keep = ppo_ref.used_samples(a, adv, w)
    h = x.astype(np.float64)[:, keep]
    for l, (wt, b) in enumerate(layers):
        y = wt @ h + b[:, None]
        act = out if l == len(layers) - 1 else hidden
        h = np.tanh(y) if act == "tanh" else np.maximum(y, 0) if act == "relu" else y
    e = (a.astype(np.float64)[:, keep] - out_scale * h) / np.exp(log_sigma)[:, None]
    logp = -0.5 * (e * e).sum(axis=0) - log_sigma.sum()
    ratio = np.exp(logp - old_full[keep])
    lo, hi = ppo_ref.bounds(CLIP)
    A = adv.astype(np.float64)[keep]
    obj = np.minimum(ratio * A, np.clip(ratio, float(lo), float(hi)) * A)
    return float((w.astype(np.float64)[keep] * obj).sum()), ratio


@pytest.mark.parametrize("widths, hidden, out", [((), "tanh", "tanh"), ((3,), "tanh", "identity"), ((4, 3), "tanh", "tanh")])
def test_fp64_gradients_agree_with_central_differences_of_the_clipped_surrogate(widths, hidden, out):
    rng = np.random.RandomState(13)
    n_in, dof, S = 5, 2, 48
    layers = policy_ref.make_weights(3, n_in, widths, dof)
    layers = [(w * np.float32(20), b) for w, b in layers]            # out of the linear range of the first layer
    x = rng.randn(n_in, S).astype(np.float32)
    a = (40 * rng.randn(dof, S)).astype(np.float32)
    adv = rng.randn(S).astype(np.float32)
    adv[2] = 0
    a[1, 4] = np.nan                                                 # skipped, not poisoned
    w = rng.choice(np.array([0.0, 0.5, 1.0, 2.0], dtype=np.float32), size=S)     # (exact products with adv)
    sigma = np.array([32.0, 64.0], dtype=np.float32)                 # (1 / sigma^2 is exact in fp32)
    log_sigma = np.log(sigma.astype(np.float64))
    # old_logp: the current one (normaliser dropped, as mt_policy_eval gives it) moved by +-(0.05 .. 0.6): every class is there
    base = ppo_ref.ppo_grad(layers, x, a, adv, np.zeros(S, np.float32), sigma, hidden, out, 180.0, CLIP, weight=w)
    move = rng.uniform(0.05, 0.6, size=S) * rng.choice([-1.0, 1.0], size=S)
    old = (base["logp"] - move).astype(np.float32)
    got = ppo_ref.ppo_grad(layers, x, a, adv, old, sigma, hidden, out, 180.0, CLIP, weight=w)
    A = ppo_ref.advantage(adv, w)
    frac = ppo_ref.class_fractions(A, got["clipped_mask"], got["used_mask"])
    assert min(frac.values()) > 0.05, frac
    assert 0 < got["clipped"] < got["used"] < S
    lo, hi = ppo_ref.bounds(CLIP)
    r = got["ratio"][got["used_mask"]]
    assert np.minimum(np.abs(r - float(lo)), np.abs(r - float(hi))).min() > 1e-3   # no sample near a kink of the objective
    assert np.isfinite(got["grad"]).all() and np.isfinite(got["sigma_grad"]).all()
    assert (got["grad_abs"] >= np.abs(got["grad"]) * (1 - 1e-12)).all()
    assert (got["sigma_abs"] >= np.abs(got["sigma_grad"]) * (1 - 1e-12)).all()
    assert got["kl"] >= 0 and got["kl_abs"] >= got["kl"]

    shapes = [wt.shape for wt, _ in layers]
    theta = pg_ref.flatten(layers).astype(np.float64)
    old_full = old.astype(np.float64) - log_sigma.sum()              # the old density with ITS normaliser (sigma_old = sigma)

    def J(th, ls):
        lay = [(wt.astype(np.float64), b.astype(np.float64)) for wt, b in pg_ref.unflatten(th, shapes)]
        return _surrogate64(lay, ls, x, a, adv, w, old_full, hidden, out, 180.0)

    value, ratio = J(theta, log_sigma)
    np.testing.assert_allclose(ratio, r, rtol=1e-6)                  # (the restatement rounds 1 / sigma^2 to fp32)
    np.testing.assert_allclose(got["loss"], value, rtol=1e-6)
    fd = np.empty_like(theta)
    for i in range(theta.size):
        step = 1e-6 * max(1.0, abs(theta[i]))
        th_p, th_m = theta.copy(), theta.copy()
        th_p[i] += step
        th_m[i] -= step
        fd[i] = (J(th_p, log_sigma)[0] - J(th_m, log_sigma)[0]) / (2 * step)
    np.testing.assert_allclose(got["grad"], fd, rtol=2e-5, atol=2e-5 * float(np.abs(got["grad"]).max()))
    fds = np.empty(dof)
    for j in range(dof):
        step = 1e-6
        ls_p, ls_m = log_sigma.copy(), log_sigma.copy()
        ls_p[j] += step
        ls_m[j] -= step
        fds[j] = (J(theta, ls_p)[0] - J(theta, ls_m)[0]) / (2 * step)
    np.testing.assert_allclose(got["sigma_grad"], fds, rtol=2e-5, atol=2e-5 * float(np.abs(got["sigma_grad"]).max()))


def test_shift_stands_for_a_changed_sigma():
    """logp drops the normaliser, so a sigma changed since old_logp was taken enters x as sum_j log(sigma_old_j / sigma_j)."""
    rng = np.random.RandomState(4)
    n_in, dof, S = 5, 2, 32
    layers = policy_ref.make_weights(3, n_in, (4,), dof)
    x = rng.randn(n_in, S).astype(np.float32)
    a = (40 * rng.randn(dof, S)).astype(np.float32)
    adv = rng.randn(S).astype(np.float32)
    sigma_old, sigma = np.array([30.0, 45.0]), np.array([33.0, 40.0])
    old = ppo_ref.forward(layers, x, a, sigma_old, "tanh", "tanh", 180.0)[2].astype(np.float32)
    shift = float(np.log(sigma_old / sigma).sum())
    got = ppo_ref.ppo_grad(layers, x, a, adv, old, sigma, "tanh", "tanh", 180.0, CLIP, shift=shift)
    mu_e = ppo_ref.forward(layers, x, a, np.ones(dof), "tanh", "tanh", 180.0)[0]      # a - mu
    full = lambda s: -0.5 * ((mu_e / s[:, None]) ** 2).sum(axis=0) - np.log(s).sum()
    np.testing.assert_allclose(got["ratio"], np.exp(full(sigma) - full(sigma_old)), rtol=1e-5)


def test_fp32_restatement_is_close_to_fp64_and_the_fp32_coefficient_is_its_own_function():
    rng = np.random.RandomState(11)
    n_in, dof, S = 21, 4, 512
    layers = policy_ref.make_weights(5, n_in, (33, 64), dof)
    x = (30 * rng.randn(n_in, S)).astype(np.float32)
    a = (60 * rng.randn(dof, S)).astype(np.float32)
    adv = rng.randn(S).astype(np.float32)
    adv[rng.rand(S) < 0.1] = 0
    sigma = np.full(dof, 40.0)
    base = ppo_ref.ppo_grad(layers, x, a, adv, np.zeros(S, np.float32), sigma, "tanh", "tanh", 180.0, CLIP)
    old = (base["logp"] - 0.4 * rng.randn(S)).astype(np.float32)
    g64 = ppo_ref.ppo_grad(layers, x, a, adv, old, sigma, "tanh", "tanh", 180.0, CLIP)
    g32 = ppo_ref.ppo_grad(layers, x, a, adv, old, sigma, "tanh", "tanh", 180.0, CLIP, dtype=np.float32,
                           decide_ratio=g64["ratio"].astype(np.float32))
    assert g32["grad"].dtype == np.float32 and g32["used"] == g64["used"] and g32["clipped"] == g64["clipped"]
    live = g64["grad_abs"] > 0
    assert (np.abs(g32["grad"] - g64["grad"])[live] / g64["grad_abs"][live]).max() < 1e-4
    assert abs(g32["kl"] - g64["kl"]) < 1e-4 * g64["kl_abs"]
    c, used, clipped = ppo_ref.coef32(g32["ratio"], adv, None, g32["used_mask"], CLIP)
    assert used == g32["used"] and c.dtype == np.float32
    free = g32["used_mask"] & ~ppo_ref.decide(g32["ratio"], adv, g32["used_mask"], CLIP)
    np.testing.assert_array_equal(c[free], (g32["ratio"] * adv)[free])
    assert not c[~free].any() and clipped == int((g32["used_mask"] & ~free).sum())
    # clip = 0 never clips
    assert ppo_ref.coef32(g32["ratio"], adv, None, g32["used_mask"], 0.0)[2] == 0
