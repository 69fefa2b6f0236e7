"""Host restatement of mt_gae, of mt_policy_eval's log-probability and of mt_value_grad (include/manytor_hip.h): the GAE
recurrence and the logp sequence in exact fp32 (pg_ref.fma32 where the kernels fuse), the value head's gradient as
pg_ref.policy_grad with one output, sigma = 1 and the target in the action's place.  Shared by the CPU and the GPU tests of
the three calls."""
import numpy as np

import pg_ref
from cem_ref import unusable

# max |V_kernel - V_fp64| of a ONE-output identity head at out_scale = 1 over the seven configs of
# tests/test_gpu_policy_eval.py::test_value_head_against_fp64 (it prints the figure per config): measured on an MI355X,
# 9.5e-8 (width 1) to 4.648e-7 (K = 32, IN = 100); the plain fp32 numpy restatement (policy_ref.mlp with dtype=np.float32)
# reaches 6.7e-8 to 5.154e-7 against fp64 on the same inputs (its maximum on the one-layer config).
# The gate is 4 x the measured maximum -- the populations are a few thousand samples per config, so the tail needs room
# (policy_ref.ACTION_TOL_DEG's reasoning) -- and may be no more than 16 x the numpy figure.
VALUE_MEASURED = 4.648e-7
VALUE_REF32_MEASURED = 5.154e-7
VALUE_TOL = 4.0 * VALUE_MEASURED
assert VALUE_TOL <= 16.0 * VALUE_REF32_MEASURED


def gae(reward, done, value, last_value=None, gamma=0.99, lam=0.95, mask_after_done=False):
    """reward (T, n) int8, done (T, n) uint8, value (T, n) f32, last_value (n,) f32 or None -> (adv, ret, weight), each
    (T, n) float32, in mt_gae's own arithmetic: gl = fl(gamma * lam); delta = fma(gamma, 0 if done_t else V_t+1, r_t) - V_t;
    A_t = fma(gl, 0 if done_t else A_t+1, delta); ret_t = A_t + V_t; weight 1.  With mask_after_done the steps behind an
    env's first done hold exactly 0 in all three and do not enter the recurrence (their values are never looked at)."""
    reward, done = np.asarray(reward), np.asarray(done) != 0
    value = np.asarray(value, dtype=np.float32)
    T, n = reward.shape
    g = np.float32(gamma)
    gl = np.float32(g * np.float32(lam))
    zero = np.float32(0)
    behind = np.zeros((T, n), dtype=bool)
    if mask_after_done and T:
        behind[1:] = np.cumsum(done, axis=0)[:-1] > 0
    adv, ret, weight = (np.zeros((T, n), dtype=np.float32) for _ in range(3))
    A = np.zeros(n, dtype=np.float32)
    Vn = np.zeros(n, dtype=np.float32) if last_value is None else np.asarray(last_value, dtype=np.float32)
    for t in range(T - 1, -1, -1):
        live = ~behind[t]
        V = np.where(live, value[t], zero)                           # (a masked step's value may be anything, NaN included)
        delta = (pg_ref.fma32(g, np.where(done[t], zero, Vn), reward[t].astype(np.float32)) - V).astype(np.float32)
        new = pg_ref.fma32(gl, np.where(done[t], zero, A), delta)
        A, Vn = np.where(live, new, A), np.where(live, V, Vn)
        adv[t] = np.where(live, new, zero)
        ret[t] = np.where(live, (new + V).astype(np.float32), zero)
        weight[t] = live
    return adv, ret, weight


def logp(mean, a, sigma):
    """mean, a (..., D, n) f32, sigma (D,) -> (..., n) float32 in mt_policy_eval's (and policy_grad_kernel's) sequence:
    inv_var_j = fl32(1 / sigma_j^2) formed in double; e = a_j - mu_j; d = e * inv_var_j; lp = fma(e, d, lp), ascending j;
    -0.5f * lp.  A sample with an unusable a_j gets exactly 0."""
    mean, a = np.asarray(mean, dtype=np.float32), np.asarray(a, dtype=np.float32)
    D = mean.shape[-2]
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float32), (D,))
    inv_var = (1.0 / (sigma.astype(np.float64) ** 2)).astype(np.float32)
    bad = unusable(a).any(axis=-2)
    lp = np.zeros(bad.shape, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(D):
            e = np.where(bad, np.float32(0), a[..., j, :] - mean[..., j, :]).astype(np.float32)
            d = (e * inv_var[j]).astype(np.float32)
            lp = pg_ref.fma32(e, d, lp)
    return np.where(bad, np.float32(0), np.float32(-0.5) * lp).astype(np.float32)


def value_grad(layers, x, target, c, hidden, out, out_scale, scale=1.0, dtype=np.float64):
    """x (IN, S), target (S,), c (S,) -> (grad (P_v,), abs_sum (P_v,), loss) for the one-output head `layers`:
    grad = scale * sum_s c_s (R_s - V_s) dV_s/dtheta, loss = scale * sum_s c_s (-1/2 (R_s - V_s)^2) -- pg_ref.policy_grad
    with D = 1, sigma = 1 and a = target, its skip rule included (c == 0 or an unusable target)."""
    assert layers[-1][0].shape[0] == 1
    return pg_ref.policy_grad(layers, x, np.asarray(target, dtype=np.float32)[None], c, np.ones(1, dtype=np.float32), hidden, out,
                              out_scale, scale=scale, dtype=dtype)
