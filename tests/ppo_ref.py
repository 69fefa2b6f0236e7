"""Host restatement of mt_ppo_grad (include/manytor_hip.h): PPO's clipped surrogate, its gradient in theta (through
pg_ref.policy_grad with the coefficient c of every sample) and in log sigma, the k3 KL estimate and the counts -- fp64 on the
fp32 inputs, or fp32 throughout -- with the skip rule and the absolute sums that bound an fp32 reduction.  Shared by the CPU
and the GPU tests of the call."""
import numpy as np

import pg_ref
from cem_ref import unusable

MAX_LOG_RATIO = 20.0                    # MT_PPO_MAX_LOG_RATIO

# max over used samples of |ratio_out - exp_fp64(x)| / exp_fp64(x) / (1 + |x|), x the kernel's own fp32 log-ratio, over the
# cases of tests/test_gpu_ppo_grad.py::test_ratio_against_fp64_exp (it prints the figure per case).  The formula -- the
# hardware's exp2 (1 ulp) of the rounded product x * log2(e) -- gives at most about 1.2e-7 + 9e-8 |x|, so 1.2e-7 per
# (1 + |x|).  Measured on an MI355X: 5.0e-8 to 7.32e-8 over the seven cases (237 to 1627 used samples each, |x| up to 3.5),
# and within the gate at the clamp, |x| = 20.  The gate is 4 x the measured maximum and may be no more than 2^-20: a larger
# figure means another formula.
RATIO_MEASURED = 7.32e-8
RATIO_TOL = 4.0 * RATIO_MEASURED
assert RATIO_TOL <= 2.0 ** -20


def bounds(clip):
    """(lo, hi): the fp32 nearest to 1 -+ clip, formed in double from the fp32 clip, as the host does."""
    c = float(np.float32(clip))
    return np.float32(1.0 - c), np.float32(1.0 + c)


def advantage(adv, weight=None):
    """A = fl32(weight * adv) (adv itself without weight)."""
    adv = np.asarray(adv, dtype=np.float32)
    return adv if weight is None else (np.asarray(weight, dtype=np.float32) * adv).astype(np.float32)


def used_samples(a, adv, weight=None):
    """(S,) bool: A != 0 and every a_j usable."""
    return (advantage(adv, weight) != 0) & ~unusable(np.asarray(a, dtype=np.float32)).any(axis=0)


def log_ratio(new_logp, old_logp, shift=0.0):
    """The kernel's fp32 x: two fp32 adds, then the clamp."""
    x = (np.asarray(new_logp, dtype=np.float32) - np.asarray(old_logp, dtype=np.float32)).astype(np.float32) + np.float32(shift)
    return np.minimum(np.maximum(x.astype(np.float32), np.float32(-MAX_LOG_RATIO)), np.float32(MAX_LOG_RATIO))


def decide(ratio, A, used, clip):
    """(S,) bool: the clipped samples, from `ratio` compared with the fp32 bounds in ratio's own precision."""
    lo, hi = bounds(clip)
    if float(np.float32(clip)) == 0.0:
        return np.zeros(A.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        return used & (((A > 0) & (ratio > ratio.dtype.type(hi))) | ((A < 0) & (ratio < ratio.dtype.type(lo))))


def coef32(ratio, adv, weight, used, clip):
    """The kernel's fp32 function of its own ratio: (coef (S,) f32, used count, clipped count)."""
    ratio = np.asarray(ratio, dtype=np.float32)
    A = advantage(adv, weight)
    clipped = decide(ratio, A, used, clip)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.where(used & ~clipped, (ratio * A).astype(np.float32), np.float32(0)).astype(np.float32)
    return c, int(used.sum()), int(clipped.sum())


def forward(layers, x, a, sigma, hidden, out, out_scale, dtype=np.float64):
    """x (IN, S), a (D, S) -> (e, d, logp) in `dtype`: e = a - mu, d = e * inv_var (the fp32 inv_var the kernel is given),
    logp = -1/2 sum_j e_j d_j."""
    f = lambda v: np.asarray(v, dtype=np.float32).astype(dtype)
    inv_var = (1.0 / (f(sigma).astype(np.float64) ** 2)).astype(np.float32).astype(dtype)[:, None]
    h = f(x)
    for l, (w, b) in enumerate(layers):
        y = f(w) @ h + f(b)[:, None]
        h = pg_ref._ACT[out if l == len(layers) - 1 else hidden](y).astype(dtype)
    e = f(a) - dtype(out_scale) * h
    d = e * inv_var
    return e, d, dtype(-0.5) * (e * d).sum(axis=0)


def ppo_grad(layers, x, a, adv, old_logp, sigma, hidden, out, out_scale, clip, weight=None, shift=0.0, scale=1.0,
             dtype=np.float64, log_ratio_in=None, decide_ratio=None):
    """x (IN, S), a (D, S), adv / old_logp / weight (S,), sigma (D,) -> a dict, floats in `dtype`:
      grad, grad_abs (P,)    scale * sum_s c_s dlogp_s/dtheta and sum_s |c_s dlogp_s/dtheta_i| (pg_ref.policy_grad with coef = c)
      loss, loss_abs         scale * sum obj, sum |obj|
      kl, kl_abs             scale * sum (ratio - 1) - x over the used samples, sum |ratio - 1| + |x|
      sigma_grad, sigma_abs  (D,) scale * sum c (e_j d_j - 1), sum |c| (|e_j d_j| + 1)
      used, clipped          counts;  x, ratio, coef (S,): 0 on skipped samples
    log_ratio_in: the fp32 x of every sample to take instead of the restatement's own (the kernel's, rebuilt from
    mt_policy_eval's logp); decide_ratio: the ratio the clip decisions are taken from (the kernel's own), else this one's.
    Skipped samples are taken out before any arithmetic sees them."""
    a = np.asarray(a, dtype=np.float32)
    A32 = advantage(adv, weight)
    used = used_samples(a, adv, weight)
    S = A32.shape[0]
    lo, hi = bounds(clip)
    xs = np.asarray(x, dtype=np.float32)[:, used]
    e, d, logp = forward(layers, xs, a[:, used], sigma, hidden, out, out_scale, dtype)
    A = A32[used].astype(dtype)
    if log_ratio_in is None:
        lx = (logp - np.asarray(old_logp, dtype=np.float32)[used].astype(dtype)) + dtype(shift)
        lx = np.minimum(np.maximum(lx, dtype(-MAX_LOG_RATIO)), dtype(MAX_LOG_RATIO))
    else:
        lx = np.asarray(log_ratio_in, dtype=np.float32)[used].astype(dtype)
    ratio = np.exp(lx).astype(dtype)
    rdec = ratio if decide_ratio is None else np.asarray(decide_ratio)[used]
    clipped = decide(rdec, A32[used] if rdec.dtype == np.float32 else A, np.ones(A.shape, dtype=bool), clip)
    ra = ratio * A
    c = np.where(clipped, dtype(0), ra).astype(dtype)
    obj = np.where(clipped, np.where(A > 0, dtype(hi), dtype(lo)) * A, ra)

    def full(v):
        z = np.zeros(S, dtype=v.dtype)
        z[used] = v
        return z

    cfull = full(c)
    # (pg_ref rounds its coef to fp32: 6e-8 relative, far inside what the sums are held to)
    xin = np.array(x, dtype=np.float32)
    ain = np.array(a, dtype=np.float32)
    xin[:, ~used] = 0
    ain[:, ~used] = 0
    grad, grad_abs, _ = pg_ref.policy_grad(layers, xin, ain, cfull, sigma, hidden, out, out_scale, scale=scale, dtype=dtype)
    k = (ratio - dtype(1)) - lx
    sg = c[None] * (e * d - dtype(1))
    return {
        "grad": grad, "grad_abs": grad_abs,
        "loss": dtype(scale) * obj.sum(dtype=dtype), "loss_abs": np.abs(obj).sum(dtype=dtype),
        "kl": dtype(scale) * k.sum(dtype=dtype), "kl_abs": (np.abs(ratio - dtype(1)) + np.abs(lx)).sum(dtype=dtype),
        "sigma_grad": dtype(scale) * sg.sum(axis=1, dtype=dtype), "sigma_abs": (np.abs(c)[None] * (np.abs(e * d) + dtype(1))).sum(axis=1),
        "used": int(used.sum()), "clipped": int(clipped.sum()), "used_mask": used, "clipped_mask": full(clipped.astype(dtype)) != 0,
        "x": full(lx), "ratio": full(ratio), "coef": cfull, "logp": full(logp),
    }


def class_fractions(A, ratio_or_clipped, used):
    """The share of the used samples in each of the four classes (A > 0 / A < 0) x (clipped / not): a dict."""
    n = max(int(used.sum()), 1)
    cl = ratio_or_clipped
    return {"pos_clipped": float((used & (A > 0) & cl).sum()) / n, "pos_free": float((used & (A > 0) & ~cl).sum()) / n,
            "neg_clipped": float((used & (A < 0) & cl).sum()) / n, "neg_free": float((used & (A < 0) & ~cl).sum()) / n}
