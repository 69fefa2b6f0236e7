#!/usr/bin/env python3
"""mt_policy_grad against the replay it replaces: device time of the weighted log-likelihood gradient over the logs of T = 20
steps, at 65 536 / 1 048 576 arms of the reference arm (D = 4, K = 7), for policies of (L, width) = (1, -), (2, 32), (3, 32),
(3, 64): tanh hidden layers, a tanh output scaled to +-179 degrees, the same weights and the same logs on both sides.

Per point, on ONE handle running on torch's stream, interleaved, REPS repeats after a warm-up, timed between two HIP events
on that stream (tools/policy_rollout_sweep.py's protocol):
  fused   : one mt_policy_grad through the C entry point (two launches)
  torch   : a torch.nn.Sequential with the same weights replays the (T N, IN) observations under autograd, the same loss
            scale * sum c * -1/2 sum_j ((a - mu) / sigma)^2, loss.backward()
Memory: the call's workspace against torch's peak allocated bytes above what was allocated before the replay.
A point counts as faster / slower only if the medians differ by more than the larger spread (max - min over the repeats).

    python tools/policy_grad_sweep.py [sizes ...] > profiles/policy_grad_sweep.json"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import manytor_amd as m  # noqa: E402

T, K = 20, 7
POLICIES = ((1, 0), (2, 32), (3, 32), (3, 64))
REPS = 9
SEED = 0x7A9E
OUT_SCALE = 179.0
SIGMA = 15.0


def stats(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4), "spread": round(s[-1] - s[0], 4)}


def make_layers(eng, n_layers, width):
    dev = torch.device("cuda", eng.device)
    g = torch.Generator(device=dev)
    g.manual_seed(SEED)
    n_in = 3 * K
    sizes = [n_in] + [width] * (n_layers - 1) + [eng.dof]
    return [(torch.randn(o, i, device=dev, generator=g) * (1.0 / (60.0 * n_in ** 0.5) if l == 0 else i ** -0.5),
             torch.randn(o, device=dev, generator=g) * 0.1) for l, (i, o) in enumerate(zip(sizes[:-1], sizes[1:]))]


def fused_call(eng, layers, log, coef, grad):
    arg = m.lib.MtPolicyGrad()
    arg.struct_size, arg.n_steps, arg.n_layers = C.sizeof(m.lib.MtPolicyGrad), T, len(layers)
    for l, (w, b) in enumerate(layers):
        arg.weight[l], arg.bias[l] = w.data_ptr(), b.data_ptr()
        if l < len(layers) - 1:
            arg.width[l] = int(w.shape[0])
    arg.hidden_act = arg.out_act = m.lib.ACT_TANH
    arg.out_scale, arg.scale = OUT_SCALE, 1.0 / eng.n_envs
    arg.sigma[:] = [SIGMA] * m.lib.MT_MAX_DOF
    arg.obs, arg.action, arg.coef = log["observations"].data_ptr(), log["actions"].data_ptr(), coef.data_ptr()
    arg.obs_ld = arg.act_ld = arg.coef_ld = eng.n_envs
    need = int(eng._lib.mt_policy_grad_workspace(eng._h, len(layers), arg.width, 0, T))
    ws = torch.empty(need // 4, dtype=torch.float32, device=grad.device)
    arg.grad_out, arg.workspace, arg.workspace_bytes = grad.data_ptr(), ws.data_ptr(), need

    def run():
        m.lib.check(eng._lib.mt_policy_grad(eng._h, C.byref(arg)), eng._h)
    run.keep = ws
    return run, need


def torch_call(eng, layers, log, coef):
    mods = []
    for l, (w, b) in enumerate(layers):
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
    c = coef.reshape(T * n)

    def run():
        for p in net.parameters():
            p.grad = None
        e = (a - OUT_SCALE * net(x)) / SIGMA
        loss = (c * (-0.5 * (e * e).sum(dim=1))).sum() / n
        loss.backward()
    run.net = net
    return run


def timed(eng, fn):
    torch.cuda.synchronize(eng.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)          # ms per gradient of the whole batch


def measure(n, n_layers, width):
    eng = m.StepEngine(n, K)
    eng.use_torch_stream()
    eng.reset_random(SEED, 0)
    layers = make_layers(eng, n_layers, width)
    log = eng.rollout_policy(layers, T, sigma=SIGMA, seed=SEED, out_scale=OUT_SCALE, log=True, actions=True, observations=True)
    coef = eng.reward_to_go(log["reward"], log["done"], 0.95, 0.0, mask_after_done=True)
    grad = torch.zeros(eng.policy_size((width,) * (n_layers - 1)), device=coef.device)
    fused, workspace = fused_call(eng, layers, log, coef, grad)
    replay = torch_call(eng, layers, log, coef)
    paths = {"fused": fused, "torch": replay}
    for fn in paths.values():
        for _ in range(2):
            timed(eng, fn)
    # the two gradients agree (the fused one against torch's, relative to the largest entry)
    theirs = torch.cat([p.grad.reshape(-1) for p in replay.net.parameters()])
    agree = float((grad - theirs).abs().max() / theirs.abs().max())
    torch.cuda.synchronize(eng.device)
    base = torch.cuda.memory_allocated(eng.device)
    torch.cuda.reset_peak_memory_stats(eng.device)
    timed(eng, replay)
    peak = torch.cuda.max_memory_allocated(eng.device) - base
    ms = {k: [] for k in paths}
    for _ in range(REPS):
        for k, fn in paths.items():
            ms[k].append(timed(eng, fn))
    out = {k: stats(v) for k, v in ms.items()}
    a, b = out["fused"], out["torch"]
    out["torch_over_fused"] = round(b["median"] / a["median"], 3)
    out["separated"] = bool(abs(a["median"] - b["median"]) > max(a["spread"], b["spread"]))
    out["fused_ns_per_sample"] = round(a["median"] * 1e6 / (n * T), 4)
    out["workspace_bytes"] = workspace
    out["torch_peak_bytes"] = int(peak)
    out["max_rel_difference"] = agree
    eng.close()
    del layers, paths, log, coef, fused, replay
    torch.cuda.empty_cache()
    return out


def main():
    sizes = [int(v) for v in sys.argv[1:]] or [65536, 1048576]
    res = {"T": T, "K": K, "table": "ref4", "reps": REPS, "unit": "device ms per gradient of the whole batch (T x N samples)"}
    for n in sizes:
        res[str(n)] = {}
        for n_layers, width in POLICIES:
            key = f"L{n_layers}" + (f"_w{width}" if n_layers > 1 else "")
            res[str(n)][key] = measure(n, n_layers, width)
            print(f"# n={n} {key}: {json.dumps(res[str(n)][key])}", file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
