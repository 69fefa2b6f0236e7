"""Host restatement of mt_policy_grad and mt_reward_to_go (include/manytor_hip.h): the policy's forward and backward pass in
numpy -- fp64 on the fp32 inputs, or fp32 throughout -- with the skip rule, the per-parameter absolute sum that bounds an
fp32 reduction, and the reward-to-go recurrence in exact fp32 (one fused multiply-add per step).  Shared by the CPU and the
GPU tests of the two calls."""
import numpy as np

from cem_ref import unusable

# max over parameters of |grad_kernel - grad_fp64| / sum_s |c_s dlogp_s/dtheta_i| over the eighteen cases of
# tests/test_gpu_policy_grad.py::test_gradient_against_fp64 (it prints the figure per case): measured on an MI355X, 5.9e-8 to
# 1.6e-6 in seventeen of them and 6.39e-6 in the largest (D = 7, a relu layer of 5, real logs); the fp32 restatement below
# reaches 4.6e-8 to 1.5e-6 and 4.01e-6 against fp64 on the same inputs, case by case.  The gate is 4 x the maximum: the
# populations are a few thousand samples per shape, so the tail needs room (policy_ref.ACTION_TOL_DEG's reasoning), and it
# may be no more than 16 x what plain fp32 numpy reaches.
GRAD_MEASURED = 6.39e-6
REF32_MEASURED = 4.01e-6
GRAD_TOL = 4.0 * GRAD_MEASURED
assert GRAD_TOL <= 16.0 * REF32_MEASURED

_ACT = {
    "identity": lambda y: y,
    "tanh": np.tanh,
    "relu": lambda y: np.maximum(y, 0),
}
_SLOPE = {       # from the forward VALUE h
    "identity": lambda h: np.ones_like(h),
    "tanh": lambda h: 1 - h * h,
    "relu": lambda h: (h > 0).astype(h.dtype),
}


def usable_samples(a, c):
    """(S,) bool: the samples that count -- c != 0 and every a_j usable (finite, within +-32768 degrees)."""
    a = np.asarray(a, dtype=np.float32)
    return (np.asarray(c, dtype=np.float32) != 0) & ~unusable(a).any(axis=0)


def policy_grad(layers, x, a, c, sigma, hidden, out, out_scale, scale=1.0, dtype=np.float64):
    """x (IN, S), a (D, S), c (S,), sigma (D,) -> (grad (P,), abs_sum (P,), loss), all in `dtype`:
    grad = scale * sum_s c_s dlogp_s/dtheta in the flat layout W0|b0|W1|b1|..., logp_s = -1/2 sum_j ((a_j - mu_j) / sigma_j)^2;
    abs_sum_i = sum_s |c_s dlogp_s/dtheta_i| (without scale); loss = scale * sum_s c_s logp_s.  Skipped samples are taken out
    before any arithmetic sees them."""
    keep = usable_samples(a, c)
    f = lambda v: np.asarray(v, dtype=np.float32).astype(dtype)
    x, a, c = f(x)[:, keep], f(a)[:, keep], f(c)[keep]
    inv_var = (1.0 / (f(sigma).astype(np.float64) ** 2)).astype(np.float32).astype(dtype)[:, None]   # the fp32 the kernel is given
    hs, h = [x], x
    for l, (w, b) in enumerate(layers):
        y = f(w) @ h + f(b)[:, None]
        h = _ACT[out if l == len(layers) - 1 else hidden](y).astype(dtype)
        hs.append(h)
    e = a - dtype(out_scale) * hs[-1]
    d = e * inv_var
    loss = dtype(scale) * (c * (dtype(-0.5) * (e * d).sum(axis=0))).sum()
    delta = (c[None] * d) * dtype(out_scale) * _SLOPE[out](hs[-1])
    grads, sums = [], []
    for l in range(len(layers) - 1, -1, -1):
        grads[:0] = [(delta @ hs[l].T).ravel(), delta.sum(axis=1)]
        sums[:0] = [(np.abs(delta) @ np.abs(hs[l]).T).ravel(), np.abs(delta).sum(axis=1)]
        if l:
            delta = (f(layers[l][0]).T @ delta) * _SLOPE[hidden](hs[l])
    return (dtype(scale) * np.concatenate(grads)).astype(dtype), np.concatenate(sums).astype(dtype), dtype(loss)


def flatten(layers):
    return np.concatenate([np.asarray(t, dtype=np.float32).ravel() for pair in layers for t in pair])


def unflatten(theta, shapes):
    out, off = [], 0
    for o, i in shapes:
        out.append((theta[off:off + o * i].reshape(o, i), theta[off + o * i:off + o * i + o]))
        off += o * i + o
    return out


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for fp32 arrays: the product of two fp32 is exact in fp64; the sum is formed in
    fp64 with its rounding error recovered (TwoSum) and rounded TO ODD, which makes the final rounding to fp32 the correctly
    rounded one (53 >= 2 * 24 + 2 bits)."""
    p = np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    odd = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return odd.astype(np.float32)


def reward_to_go(reward, done, gamma=1.0, baseline=0.0, mask_after_done=False):
    """reward (T, n) int8, done (T, n) uint8 -> (T, n) float32: R_t = fma(gamma, 0 if done_t else R_t+1, r_t), R_T = 0;
    out = R_t - baseline; with mask_after_done exactly 0 behind an env's first done."""
    reward, done = np.asarray(reward), np.asarray(done) != 0
    T, n = reward.shape
    out = np.zeros((T, n), dtype=np.float32)
    g, base = np.float32(gamma), np.float32(baseline)
    behind = np.zeros((T, n), dtype=bool)
    if mask_after_done and T:
        behind[1:] = np.cumsum(done, axis=0)[:-1] > 0
    R = np.zeros(n, dtype=np.float32)
    for t in range(T - 1, -1, -1):
        new = fma32(g, np.where(done[t], np.float32(0), R), reward[t].astype(np.float32))
        R = np.where(behind[t], R, new)
        out[t] = np.where(behind[t], np.float32(0), new - base)
    return out
