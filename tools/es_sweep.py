#!/usr/bin/env python3
"""mt_es against the parts a user writes without it: device time of ONE evolution-strategies generation (M members, T = 20
steps, rank shaping) at 65 536 / 1 048 576 arms of the reference arm (D = 4, K = 7), M = 64 / 1024, for policies of
(L, width) = (1, -), (2, 32), (3, 64): tanh hidden layers, a tanh output scaled to +-179 degrees.

Per point, on ONE handle running on torch's stream, interleaved, REPS repeats after a warm-up, timed between two HIP events
on that stream (tools/policy_rollout_sweep.py's protocol):
  es     : one mt_es through the C entry point (sample, score, update: four launches), nothing logged
  parts  : torch.randn (M / 2, P) noise, materialised, and the (M, P) population from it;
           T x (mt_observe; torch.baddbmm + tanh per layer over the (M, ., G) views of the observation rows, the last into
           the staged actions; mt_step);
           torch member means, mid-ranks by an (M, M) comparison, and the (M,) @ (M, P) update
and, for the cost of per-member weights alone, at the same shape and nothing logged:
  population : one mt_rollout_population of T steps (M weight sets)
  policy     : one mt_rollout_policy of T steps (one weight set: member 0's)
Every timed region starts from a freshly reset, idle handle.  A pair counts as separated only if the medians differ by more
than the larger spread (max - min over the repeats).

    python tools/es_sweep.py [sizes ...] > profiles/es_sweep.json"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import manytor_amd as m  # noqa: E402

T, K = 20, 7
POLICIES = ((1, ()), (2, (32,)), (3, (64, 64)))
MEMBERS = (64, 1024)
REPS = 9
SEED = 0x7A9E
OUT_SCALE = 179.0
SIGMA, LR = 0.02, 0.05


def stats(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4), "spread": round(s[-1] - s[0], 4)}


def make_theta(eng, widths):
    dev = torch.device("cuda", eng.device)
    g = torch.Generator(device=dev)
    g.manual_seed(SEED)
    n_in = 3 * K
    sizes = [n_in] + list(widths) + [eng.dof]
    layers = [(torch.randn(o, i, device=dev, generator=g) * (1.0 / (60.0 * n_in ** 0.5) if l == 0 else i ** -0.5),
               torch.randn(o, device=dev, generator=g) * 0.1) for l, (i, o) in enumerate(zip(sizes[:-1], sizes[1:]))]
    return eng.flatten_policy(layers)


def population_arg(eng, widths, members, pop, ret, fit):
    p = m.lib.MtPopulation()
    p.struct_size, p.n_steps, p.n_members, p.n_layers = C.sizeof(m.lib.MtPopulation), T, members, len(widths) + 1
    for l, w in enumerate(widths):
        p.width[l] = w
    p.hidden_act = p.out_act = m.lib.ACT_TANH
    p.pop, p.pitch = pop.data_ptr(), pop.stride(0)
    p.out_scale, p.lo, p.hi, p.seed = OUT_SCALE, -180.0, 180.0, SEED
    p.return_out = ret.data_ptr() if ret is not None else None
    p.fitness_out = fit.data_ptr() if fit is not None else None
    return p


def es_call(eng, widths, members, theta, bufs):
    arg = m.lib.MtEs()
    arg.struct_size, arg.shaping, arg.sigma, arg.lr, arg.flags = C.sizeof(m.lib.MtEs), m.lib.ES_SHAPE_RANK, SIGMA, LR, m.lib.ES_INPLACE
    arg.theta, arg.grad_out = theta.data_ptr(), bufs["grad"].data_ptr()
    arg.best_out, arg.coeff_out = bufs["best"].data_ptr(), bufs["coeff"].data_ptr()
    arg.pop = population_arg(eng, widths, members, bufs["pop"], bufs["ret"], bufs["fit"])

    def run():
        m.lib.check(eng._lib.mt_es(eng._h, C.byref(arg)), eng._h)
    return run


def population_call(eng, widths, members, bufs):
    arg = population_arg(eng, widths, members, bufs["pop"], None, None)

    def run():
        m.lib.check(eng._lib.mt_rollout_population(eng._h, C.byref(arg)), eng._h)
    return run


def policy_call(eng, widths, bufs):
    layers = eng.unflatten_policy(bufs["pop"][0], widths)
    arg = m.lib.MtPolicy()
    arg.struct_size, arg.n_steps, arg.n_layers = C.sizeof(m.lib.MtPolicy), T, len(layers)
    for l, (w, b) in enumerate(layers):
        arg.weight[l], arg.bias[l] = w.data_ptr(), b.data_ptr()
        if l < len(layers) - 1:
            arg.width[l] = int(w.shape[0])
    arg.hidden_act = arg.out_act = m.lib.ACT_TANH
    arg.out_scale, arg.lo, arg.hi, arg.seed = OUT_SCALE, -180.0, 180.0, SEED

    def run():
        m.lib.check(eng._lib.mt_rollout_policy(eng._h, C.byref(arg)), eng._h)
    return run


def parts_call(eng, widths, members, theta):
    n, d = eng.n_envs, eng.dof
    G = n // members
    obs, act = eng.device_tensor(m.lib.F_OBS), eng.device_tensor(m.lib.F_ACTIONS)
    ret = eng.device_tensor(m.lib.F_TOTAL_REWARD)
    x = obs.unflatten(1, (members, G)).permute(1, 0, 2)        # (M, IN, G)
    a = act.unflatten(1, (members, G)).permute(1, 0, 2)        # (M, D, G)
    P = theta.numel()
    shapes = [(o, i) for o, i in zip(list(widths) + [d], [3 * K] + list(widths))]

    def run():
        eps = torch.randn((members // 2, P), device=theta.device)
        eps = torch.stack((eps, -eps), dim=1).reshape(members, P)           # the (M, P) noise, materialised
        pop = theta[None] + SIGMA * eps
        layers, off = [], 0
        for o, i in shapes:
            layers.append((pop[:, off:off + o * i].view(members, o, i), pop[:, off + o * i:off + o * i + o].unsqueeze(2)))
            off += o * i + o
        for _ in range(T):
            eng.observe()
            h = x
            for w, b in layers[:-1]:
                h = torch.tanh(torch.baddbmm(b, w, h))
            w, b = layers[-1]
            a.copy_(torch.tanh(torch.baddbmm(b, w, h)).mul_(OUT_SCALE))
            eng.step()
        fit = ret.view(members, G).sum(dim=1)
        c = 2.0 * (fit[None, :] < fit[:, None]).sum(dim=1) + (fit[None, :] == fit[:, None]).sum(dim=1) - 1.0       # mid-ranks
        grad = (c @ eps) / (members * SIGMA * 2.0 * (members - 1))
        theta.add_(grad, alpha=LR)
    return run


def timed(eng, fn, episode):
    eng.reset_random(SEED, episode)
    torch.cuda.synchronize(eng.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3          # us per generation / per call of T steps


def compare(out, ours, theirs):
    a, b = out[ours], out[theirs]
    out[f"{theirs}_over_{ours}"] = round(b["median"] / a["median"], 3)
    out[f"{theirs}_vs_{ours}_separated"] = bool(abs(a["median"] - b["median"]) > max(a["spread"], b["spread"]))


def measure(n, widths, members):
    eng = m.StepEngine(n, K)
    eng.use_torch_stream()
    eng.reset_random(SEED, 0)
    dev = torch.device("cuda", eng.device)
    theta, theta_parts = make_theta(eng, widths), make_theta(eng, widths)
    P = theta.numel()
    bufs = dict(grad=torch.zeros(P, device=dev), best=torch.zeros(1, dtype=torch.int32, device=dev),
                coeff=torch.zeros(members // 2 + members, dtype=torch.int64, device=dev), pop=torch.zeros((members, P), device=dev),
                ret=torch.zeros(n, device=dev), fit=torch.zeros(members, device=dev))
    paths = {"es": es_call(eng, widths, members, theta, bufs), "parts": parts_call(eng, widths, members, theta_parts),
             "population": population_call(eng, widths, members, bufs), "policy": policy_call(eng, widths, bufs)}
    for fn in paths.values():
        for _ in range(2):
            timed(eng, fn, 0)
    us = {k: [] for k in paths}
    for r in range(REPS):
        for k, fn in paths.items():
            us[k].append(timed(eng, fn, r + 1))
    out = {k: stats(v) for k, v in us.items()}
    compare(out, "es", "parts")
    compare(out, "policy", "population")
    out["population_us_per_step"] = round(out["population"]["median"] / T, 3)
    out["policy_us_per_step"] = round(out["policy"]["median"] / T, 3)
    out["P"] = P
    eng.close()
    del paths, bufs
    torch.cuda.empty_cache()
    return out


def main():
    sizes = [int(v) for v in sys.argv[1:]] or [65536, 1048576]
    res = {"T": T, "K": K, "table": "ref4", "reps": REPS, "shaping": "rank",
           "unit": "device us per generation (es, parts) and per call of T steps (population, policy)"}
    for n in sizes:
        res[str(n)] = {}
        for n_layers, widths in POLICIES:
            for members in MEMBERS:
                key = f"L{n_layers}" + (f"_w{widths[0]}" if widths else "") + f"_M{members}"
                if (n // members) % 256:
                    res[str(n)][key] = {"not_run": f"G = {n // members} envs per member is no multiple of the rollout block (256)"}
                    continue
                res[str(n)][key] = measure(n, widths, members)
                print(f"# n={n} {key}: {json.dumps(res[str(n)][key])}", file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
