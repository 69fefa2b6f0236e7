#!/usr/bin/env python3
"""mt_policy_eval and mt_gae against the torch code they replace: device time over the logs of T = 20 steps, at 65 536 /
1 048 576 arms of the reference arm (D = 4, K = 7), for policies of (L, width) = (1, -), (2, 32), (3, 32), (3, 64): tanh
hidden layers, a tanh output scaled to +-179 degrees, the same weights and the same logs on both sides.

Per point, on ONE handle running on torch's stream, interleaved, REPS repeats after a warm-up, timed between two HIP events
on that stream (tools/policy_grad_sweep.py's protocol):
  eval       : one mt_policy_eval (mean + logp) through the C entry point (one launch)
  torch_eval : a torch.nn.Sequential with the same weights under no_grad on the (T N, IN) observations, transposed once
               outside the timed region, plus the same logp expression -1/2 sum_j ((a - mu) / sigma)^2
  gae        : one mt_gae (advantages, returns, weights; masked) through the C entry point (one launch)
  torch_gae  : the usual Python loop over T on (N,) rows, the same outputs
A point counts as faster / slower only if the medians differ by more than the larger spread (max - min over the repeats).

    python tools/policy_eval_sweep.py [sizes ...] > profiles/policy_eval_sweep.json"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import manytor_amd as m  # noqa: E402
from policy_grad_sweep import K, OUT_SCALE, POLICIES, REPS, SEED, SIGMA, T, make_layers, stats, timed  # noqa: E402

GAMMA, LAMBDA = 0.99, 0.95


def eval_call(eng, layers, log, mean, logp):
    arg = m.lib.MtPolicyEval()
    arg.struct_size, arg.n_steps, arg.n_layers = C.sizeof(m.lib.MtPolicyEval), T, len(layers)
    for l, (w, b) in enumerate(layers):
        arg.weight[l], arg.bias[l] = w.data_ptr(), b.data_ptr()
        if l < len(layers) - 1:
            arg.width[l] = int(w.shape[0])
    arg.hidden_act = arg.out_act = m.lib.ACT_TANH
    arg.out_scale = OUT_SCALE
    arg.sigma[:] = [SIGMA] * m.lib.MT_MAX_DOF
    arg.obs, arg.action, arg.mean_out, arg.logp_out = (log["observations"].data_ptr(), log["actions"].data_ptr(), mean.data_ptr(),
                                                       logp.data_ptr())
    arg.obs_ld = arg.act_ld = arg.mean_ld = arg.logp_ld = eng.n_envs

    def run():
        m.lib.check(eng._lib.mt_policy_eval(eng._h, C.byref(arg)), eng._h)
    return run


def torch_eval_call(eng, layers, log):
    mods = []
    for w, b in layers:
        lin = torch.nn.Linear(w.shape[1], w.shape[0], device=w.device)
        with torch.no_grad():
            lin.weight.copy_(w)
            lin.bias.copy_(b)
        mods += [lin, torch.nn.Tanh()]
    net = torch.nn.Sequential(*mods)
    n = eng.n_envs
    # (T, IN, N) -> (T N, IN): the replay's own layout, made once outside the timed region
    x = log["observations"].permute(0, 2, 1).reshape(T * n, -1).contiguous()
    a = log["actions"].permute(0, 2, 1).reshape(T * n, -1).contiguous()
    out = {}

    def run():
        with torch.no_grad():
            mu = OUT_SCALE * net(x)
            e = (a - mu) / SIGMA
            out["mean"], out["logp"] = mu, -0.5 * (e * e).sum(dim=1)
    run.out = out
    return run


def gae_call(eng, log, value, outs):
    arg = m.lib.MtGae()
    arg.struct_size, arg.n_steps = C.sizeof(m.lib.MtGae), T
    arg.reward_log, arg.done_log, arg.log_ld = log["reward"].data_ptr(), log["done"].data_ptr(), eng.n_envs
    arg.value, arg.value_ld = value.data_ptr(), eng.n_envs
    arg.gamma, arg.lambda_, arg.flags = GAMMA, LAMBDA, m.lib.GAE_MASK_AFTER_DONE
    arg.adv_out, arg.ret_out, arg.weight_out = (o.data_ptr() for o in outs)
    arg.adv_ld = arg.ret_ld = arg.weight_ld = eng.n_envs

    def run():
        m.lib.check(eng._lib.mt_gae(eng._h, C.byref(arg)), eng._h)
    return run


def torch_gae_call(eng, log, value):
    reward, done = log["reward"].to(torch.float32), log["done"] != 0
    out = {}

    def run():
        n = eng.n_envs
        alive = torch.cat([torch.ones((1, n), dtype=torch.bool, device=value.device), torch.cumsum(done, dim=0)[:-1] == 0])
        adv = torch.zeros_like(value)
        a = torch.zeros(n, device=value.device)
        nxt = torch.zeros(n, device=value.device)
        for t in range(T - 1, -1, -1):
            keep = (~done[t]).to(torch.float32)
            delta = reward[t] + GAMMA * keep * nxt - value[t]
            a = delta + GAMMA * LAMBDA * keep * a
            adv[t] = a
            nxt = value[t]
        w = alive.to(torch.float32)
        out["adv"], out["ret"], out["weight"] = adv * w, (adv + value) * w, w
    run.out = out
    return run


def pair(ms, ours, theirs, samples):
    a, b = stats(ms[ours]), stats(ms[theirs])
    return {ours: a, theirs: b, "torch_over_engine": round(b["median"] / a["median"], 3),
            "separated": bool(abs(a["median"] - b["median"]) > max(a["spread"], b["spread"])),
            "engine_ns_per_sample": round(a["median"] * 1e6 / samples, 4)}


def measure(n, n_layers, width, with_gae):
    eng = m.StepEngine(n, K)
    eng.use_torch_stream()
    eng.reset_random(SEED, 0)
    dev = torch.device("cuda", eng.device)
    layers = make_layers(eng, n_layers, width)
    log = eng.rollout_policy(layers, T, sigma=SIGMA, seed=SEED, out_scale=OUT_SCALE, log=True, actions=True, observations=True)
    mean, logp = torch.zeros((T, eng.dof, n), device=dev), torch.zeros((T, n), device=dev)
    paths = {"eval": eval_call(eng, layers, log, mean, logp), "torch_eval": torch_eval_call(eng, layers, log)}
    if with_gae:
        value = torch.randn((T, n), device=dev)
        outs = [torch.zeros((T, n), device=dev) for _ in range(3)]
        paths["gae"] = gae_call(eng, log, value, outs)
        paths["torch_gae"] = torch_gae_call(eng, log, value)
    for fn in paths.values():
        for _ in range(2):
            timed(eng, fn)
    theirs = paths["torch_eval"].out
    agree = {"mean_max_abs_difference_deg": float((mean.permute(0, 2, 1).reshape(T * n, -1) - theirs["mean"]).abs().max()),
             "logp_max_rel_difference": float(((logp.reshape(-1) - theirs["logp"]).abs() / theirs["logp"].abs().clamp_min(1.0)).max())}
    if with_gae:
        g = paths["torch_gae"].out
        agree["gae_max_abs_difference"] = float(max((o - g[k]).abs().max() for o, k in zip(outs, ("adv", "ret", "weight"))))
    ms = {k: [] for k in paths}
    for _ in range(REPS):
        for k, fn in paths.items():
            ms[k].append(timed(eng, fn))
    out = {"policy_eval": pair(ms, "eval", "torch_eval", n * T)}
    if with_gae:
        out["gae"] = pair(ms, "gae", "torch_gae", n * T)
    out.update(agree)
    eng.close()
    del layers, paths, log
    torch.cuda.empty_cache()
    return out


def main():
    sizes = [int(v) for v in sys.argv[1:]] or [65536, 1048576]
    res = {"T": T, "K": K, "table": "ref4", "reps": REPS, "gamma": GAMMA, "lambda": LAMBDA,
           "unit": "device ms per call over the whole batch (T x N samples)"}
    for n in sizes:
        res[str(n)] = {}
        for q, (n_layers, width) in enumerate(POLICIES):
            key = f"L{n_layers}" + (f"_w{width}" if n_layers > 1 else "")
            res[str(n)][key] = measure(n, n_layers, width, with_gae=q == 0)      # (mt_gae does not depend on the policy)
            print(f"# n={n} {key}: {json.dumps(res[str(n)][key])}", file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
