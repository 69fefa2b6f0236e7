"""numpy restatement of mt_cem's definitions (include/manytor_hip.h) -- TEST HELPER.

  * the candidate stream: Philox block -> one word per joint -> z = (sum of the word's four bytes - 510) * KZ ->
    x = mean + sigma * z (an fp32 multiply, then an fp32 add) -> handed on when unusable, else clamped to [lo, hi];
  * the elite rule: candidates ordered by (return descending, index ascending), the first E;
  * the refit: fp32, one rounding per operation, the elites summed in ascending index order.
Arrays are float32 throughout, so every numpy operation below rounds once, as the kernel's does; the sums run as loops
over the E elites, never through np.sum (pairwise).
"""
import numpy as np

from oracle.philox_ref import _ctr, philox4x32_10

TAG_PLAN = 3
KZ = np.float32(1.0 / np.sqrt(21845.0))          # the fp32 nearest to 1 / sqrt(21845)
Z_MAX = 3.4506
assert KZ.view(np.uint32) == 0x3BDDB446


def noise(words):
    """z of uint32 words (any shape), float32."""
    w = np.asarray(words, dtype=np.uint32)
    s = (w & 0xFF).astype(np.int64) + ((w >> 8) & 0xFF) + ((w >> 16) & 0xFF) + (w >> 24)
    return (s - 510).astype(np.float32) * KZ


def unusable(x):
    """kernels.h unusable_angle: NaN, +-inf or beyond +-32768 degrees, tested on the bit pattern."""
    return (np.asarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)) > np.uint32(0x47000000)


def plan_noise(seed, env_ids, draw, C, T, D, keep_mean=False):
    """(C, T, D, n) float32 z of the plan stream."""
    lo, hi = _ctr(env_ids, TAG_PLAN)
    n = lo.shape[0]
    z = np.empty((C, T, D, n), dtype=np.float32)
    for c in range(C):
        for t in range(T):
            for b in range((D + 3) // 4):
                minor = (c << 24) | (b << 16) | t
                w = philox4x32_10(lo, hi, np.uint64(draw & 0xFFFFFFFF), np.uint64(minor), seed & 0xFFFFFFFF, seed >> 32)
                for q in range(min(4, D - 4 * b)):
                    z[c, t, 4 * b + q] = noise(w[q])
    if keep_mean:
        z[0] = 0
    return z


def sample_plans(seed, env_ids, draw, C, mean, sigma, lo, hi, keep_mean=False):
    """The block mt_sample_plans writes: (C, T, D, n) float32.  mean / sigma: (T, D, n) float32."""
    mean, sigma = np.asarray(mean, dtype=np.float32), np.asarray(sigma, dtype=np.float32)
    T, D, n = mean.shape
    z = plan_noise(seed, env_ids, draw, C, T, D, keep_mean)
    with np.errstate(invalid="ignore", over="ignore"):
        sz = sigma[None] * z                      # one rounding
        x = mean[None] + sz                       # one rounding
        clamped = np.minimum(np.maximum(x, np.float32(lo)), np.float32(hi))
    return np.where(unusable(x), x, clamped).astype(np.float32)


def elite_order(returns, E):
    """(E, n) int: each env's elites -- the first E by (return descending, index ascending) -- in ASCENDING index order."""
    order = np.argsort(-np.asarray(returns, dtype=np.float64), axis=0, kind="stable")[:E]
    return np.sort(order, axis=0)


def elite_mask(returns, E):
    el = elite_order(returns, E)
    mask = np.zeros(el.shape[1], dtype=np.uint64)
    for k in range(E):
        mask |= np.uint64(1) << el[k].astype(np.uint64)
    return mask


def refit(plans, returns, E, sigma_min):
    """(mean_out, sigma_out), (T, D, n) float32 each, from the block that was scored and its (C, n) returns."""
    C, T, D, n = plans.shape
    el = elite_order(returns, E)
    inv_e = np.float32(1.0) / np.float32(E)
    cols = np.arange(n)
    x = [plans[el[k], :, :, cols].transpose(1, 2, 0) for k in range(E)]      # E x (T, D, n)
    with np.errstate(invalid="ignore", over="ignore"):
        m = x[0].copy()
        for k in range(1, E):
            m = m + x[k]
        m = m * inv_e
        d = x[0] - m
        v = d * d
        for k in range(1, E):
            d = x[k] - m
            v = v + d * d
        v = v * inv_e
        s = np.maximum(np.sqrt(v), np.float32(sigma_min))
    return m.astype(np.float32), s.astype(np.float32)
