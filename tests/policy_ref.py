"""Host restatement of mt_rollout_policy's action rule (include/manytor_hip.h): the MLP in numpy (fp64 on fp32 weights, or
fp32 throughout), the exploration-noise stream (Philox tag 4), and the clamp / unusable rule.  Shared by the CPU and the
GPU tests of the call."""
import numpy as np

from cem_ref import noise, unusable
from oracle.philox_ref import _ctr, philox4x32_10

TAG_POLICY = 4

# |tanh_kernel(y) - tanh_fp64(y)| over the hidden pre-activations of the GPU test's populations (tests/test_gpu_policy.py,
# test_tanh_error_is_within_its_constant): measured maximum 3.94e-7 on an MI355X, the fp32 rounding of the layers in front of
# the tanh included; the constant is twice that.
TANH_MEASURED = 3.94e-7
TANH_ABS_ERR = 2.0 * TANH_MEASURED
assert TANH_ABS_ERR <= 2e-6

# max |a_kernel - a_fp64| in degrees at out_scale = 180 over the same populations: measured 9.4e-5 on an MI355X (the
# numpy fp32 restatement below stays within 5.2e-5 of fp64 on the CPU); the gate is 4 x the maximum -- the populations
# are a few thousand samples per shape, so the tail needs room.
ACTION_MEASURED_DEG = 9.4e-5
ACTION_TOL_DEG = 4.0 * ACTION_MEASURED_DEG
assert ACTION_TOL_DEG <= 1e-2

_ACT = {
    "identity": lambda y: y,
    "tanh": np.tanh,
    "relu": lambda y: np.maximum(y, 0),
}


def make_weights(seed, n_in, widths, dof):
    """The GPU test's weights: seeded randn, scaled 1 / (60 sqrt(IN)) in layer 0 and 1 / sqrt(in) behind it, biases
    0.1 randn.  -> [(W (out, in) f32, b (out,) f32), ...]."""
    rng = np.random.RandomState(seed)
    layers, fan_in = [], n_in
    for l, fan_out in enumerate(tuple(widths) + (dof,)):
        scale = 1.0 / (60.0 * np.sqrt(n_in)) if l == 0 else 1.0 / np.sqrt(fan_in)
        layers.append(((rng.randn(fan_out, fan_in) * scale).astype(np.float32), (0.1 * rng.randn(fan_out)).astype(np.float32)))
        fan_in = fan_out
    return layers


def mlp(x, layers, hidden, out, out_scale, dtype=np.float64, pre_activations=None):
    """x (IN, n) -> a (D, n): out_scale * out(W_L ... hidden(W_0 x + b_0) ...) in `dtype`.  pre_activations: a list that
    receives every hidden layer's y."""
    h = np.asarray(x).astype(dtype)
    for l, (w, b) in enumerate(layers):
        y = w.astype(dtype) @ h + b.astype(dtype)[:, None]
        if l == len(layers) - 1:
            return (dtype(out_scale) * _ACT[out](y)).astype(dtype)
        if pre_activations is not None:
            pre_activations.append(y)
        h = _ACT[hidden](y).astype(dtype)


def policy_noise(seed, env_ids, draw, T, D, t0=0):
    """(T, D, n) float32 z of the policy stream: counter (e_lo, e_hi | 4 << 24, draw, (b << 16) | t)."""
    lo, hi = _ctr(env_ids, TAG_POLICY)
    z = np.empty((T, D, lo.shape[0]), dtype=np.float32)
    for t in range(T):
        for b in range((D + 3) // 4):
            w = philox4x32_10(lo, hi, np.uint64(draw & 0xFFFFFFFF), np.uint64((b << 16) | (t0 + t)), seed & 0xFFFFFFFF, seed >> 32)
            for q in range(min(4, D - 4 * b)):
                z[t, 4 * b + q] = noise(w[q])
    return z


def add_noise(a, sigma, z):
    """a + fl(sigma_j * z) in fp32 where sigma_j > 0: a multiply, then an add."""
    a = np.asarray(a, dtype=np.float32)
    sigma = np.asarray(sigma, dtype=np.float32)[:, None]
    return np.where(sigma > 0, a + sigma * np.asarray(z, dtype=np.float32), a).astype(np.float32)


def clamp(a, lo, hi):
    """The value handed to the step: as it is when unusable, else min(max(a, lo), hi)."""
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        c = np.minimum(np.maximum(a, np.float32(lo)), np.float32(hi))
    return np.where(unusable(a), a, c).astype(np.float32)
