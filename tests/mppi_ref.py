"""numpy restatement of mt_mppi's definitions (include/manytor_hip.h) -- TEST HELPER.

  * the table: W[0] = 1, W[k] = W[k-1] * decay, one fp32 rounding per entry, 2T + 1 entries;
  * the gap: k_c = (int)(best return - R_c), both integer-valued, so the subtraction is exact;
  * the weights: w_c = W[k_c];
  * the refit: fp32, one rounding per operation, every sum from +0 over c = 0, 1, ..., C-1 in order; one division.
The candidate block is cem_ref.sample_plans: mt_mppi draws from mt_cem's stream.  Arrays are float32 throughout, so every
numpy operation below rounds once, as the kernel's does; the sums run as loops over c, never through np.sum (pairwise).
"""
import numpy as np

from cem_ref import sample_plans  # noqa: F401  (the block mt_mppi scores)

MAX_STEPS = 127


def decay_of(temperature):
    """float32(exp(-1 / lambda)): what StepEngine.mppi hands to the library for temperature=lambda."""
    return np.float32(np.exp(-1.0 / float(temperature)))


def table(decay, T):
    """(2T + 1,) float32: the powers of decay by the recurrence."""
    rho = np.float32(decay)
    w = np.empty(2 * T + 1, dtype=np.float32)
    w[0] = np.float32(1.0)
    with np.errstate(under="ignore"):
        for k in range(1, 2 * T + 1):
            w[k] = w[k - 1] * rho
    return w


def gaps(returns):
    """(C, n) int: best return - return.  The returns are integer-valued floats."""
    r = np.asarray(returns, dtype=np.float32)
    top = r[0].copy()
    for c in range(1, r.shape[0]):
        top = np.maximum(top, r[c])
    return (top[None] - r).astype(np.int64)


def best(returns):
    """(best, best_return): the lowest index that reaches the maximum, and the maximum."""
    r = np.asarray(returns, dtype=np.float32)
    return np.argmax(r, axis=0).astype(np.int32), r.max(axis=0)


def weights(returns, decay, T):
    """(C, n) float32: w_c = W[gap_c]."""
    return table(decay, T)[gaps(returns)]


def weight_sum(w):
    s = np.zeros(w.shape[1], dtype=np.float32)
    for c in range(w.shape[0]):
        s = s + w[c]
    return s


def refit(plans, w, sigma_min=None):
    """(mean_out, sigma_out or None), (T, D, n) float32, from the block that was scored and its (C, n) weights."""
    C, T, D, n = plans.shape
    w = np.asarray(w, dtype=np.float32)
    s = weight_sum(w)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        a = np.zeros((T, D, n), dtype=np.float32)
        for c in range(C):
            a = a + w[c][None, None] * plans[c]
        m = a / s[None, None]
        if sigma_min is None:
            return m.astype(np.float32), None
        q = np.zeros((T, D, n), dtype=np.float32)
        for c in range(C):
            d = plans[c] - m
            q = q + w[c][None, None] * (d * d)
        sd = np.maximum(np.sqrt(q / s[None, None]), np.float32(sigma_min))
    return m.astype(np.float32), sd.astype(np.float32)
