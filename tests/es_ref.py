"""numpy restatement of the evolution-strategies definitions (include/manytor_hip.h: mt_es_sample, mt_es) -- TEST HELPER.

  * the parameter noise: pair p, parameter i -> word i & 3 of the Philox block with counter (p, 5 << 24, draw, i >> 2) ->
    byte sum - 510, an integer; eps = that * KZ (cem_ref.noise);
  * the population: theta +- fl(sigma * eps), an fp32 multiply, then an fp32 add or subtract;
  * the update: member sums, centred mid-ranks and A_i in int64 (every sum is an integer sum: no order to restate), the
    scale through float64, and one rounding per fp32 operation (arrays are float32 throughout).
"""
import numpy as np

from cem_ref import KZ
from oracle.philox_ref import _ctr, philox4x32_10

TAG_ES = 5


def byte_sums(seed, pairs, draw, P):
    """(pairs, P) int64: bytesum(p, i) - 510."""
    lo, hi = _ctr(np.arange(pairs, dtype=np.uint64), TAG_ES)
    blocks = np.arange((P + 3) // 4, dtype=np.uint64)
    w = philox4x32_10(lo[:, None], hi[:, None], np.uint64(draw & 0xFFFFFFFF), blocks[None, :], seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(w, axis=-1).reshape(pairs, -1)[:, :P].astype(np.uint32)          # word q of block b is parameter 4 b + q
    s = (words & 0xFF).astype(np.int64) + ((words >> 8) & 0xFF) + ((words >> 16) & 0xFF) + (words >> 24)
    return s - 510


def eps(seed, pairs, draw, P):
    """(pairs, P) float32 noise: one multiply."""
    return byte_sums(seed, pairs, draw, P).astype(np.float32) * KZ


def sample_population(theta, sigma, M, draw, seed):
    """(M, P) float32: row 2p = theta + fl(sigma eps_p), row 2p + 1 = theta - fl(sigma eps_p)."""
    theta = np.asarray(theta, dtype=np.float32)
    se = np.float32(sigma) * eps(seed, M // 2, draw, theta.shape[0])          # one rounding
    pop = np.empty((M, theta.shape[0]), dtype=np.float32)
    pop[0::2] = theta[None] + se
    pop[1::2] = theta[None] - se
    return pop


def member_sums(returns, M):
    """(M,) int64 S_m of the (N,) integer-valued returns."""
    r = np.asarray(returns)
    assert np.all(r == np.rint(r))
    return r.astype(np.int64).reshape(M, -1).sum(axis=1)


def mid_ranks(S):
    """c_m = 2 #{j : S_j < S_m} + #{j != m : S_j == S_m}, int64."""
    S = np.asarray(S, dtype=np.int64)
    less = (S[None, :] < S[:, None]).sum(axis=1)
    same = (S[None, :] == S[:, None]).sum(axis=1) - 1
    return (2 * less + same).astype(np.int64)


def best(S):
    return int(np.argmax(np.asarray(S, dtype=np.int64)))          # the first of the largest


def fitness(S, G):
    return np.asarray(S, dtype=np.int64).astype(np.float32) * np.float32(1.0 / G)


def scale(M, sigma, G, shaping):
    denom = float(M) * float(np.float32(sigma)) * (float(G) if shaping == "raw" else 2.0 * (M - 1))
    return np.float32(float(KZ) / denom)


def coefficients(S, shaping):
    c = np.asarray(S, dtype=np.int64) if shaping == "raw" else mid_ranks(S)
    return c[0::2] - c[1::2]


def gradient(S, sigma, G, draw, seed, P, shaping="rank"):
    """(P,) float32 grad, and the int64 A it is the conversion of."""
    M = len(S)
    d = coefficients(S, shaping)
    A = (d[:, None] * byte_sums(seed, M // 2, draw, P)).sum(axis=0)          # int64: exact
    return A.astype(np.float32) * scale(M, sigma, G, shaping), A


def apply(theta, grad, lr):
    """theta + fl(lr * grad): a multiply, then an add."""
    step = np.float32(lr) * np.asarray(grad, dtype=np.float32)
    return (np.asarray(theta, dtype=np.float32) + step).astype(np.float32)
