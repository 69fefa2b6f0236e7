#!/usr/bin/env python3
"""mt_cem against the calls it replaces: device time of ONE CEM iteration -- draw C candidate plans of T = 12 steps per arm
around (mean, sigma), score them, take each arm's E = C / 4 best, refit (mean, sigma) -- at 65 536 / 262 144 / 1 048 576
arms, C = 8, 16, 64, for the reference arm (D = 4, K = 7) and the 7-joint table.  No commit: the committing launch is the
same on every side.

Per point, on ONE handle running on torch's stream, interleaved, REPS repeats after a warm-up, timed between two HIP events
on that stream:
  cem     : one mt_cem through the C entry point (refit out of place), outputs allocated outside the region
  torch   : what the library offered before -- torch.randn over (C, T, D, N), scale by sigma, add the mean, clamp; mt_shoot
            with returns_out; torch.topk over (C, N); the advanced-index gather of E plans per arm; mean and std
  sampled : the same with mt_sample_plans in place of the torch draw
Every timed region starts from a freshly reset, idle handle.  A point counts as faster / slower only if the medians differ
by more than the larger spread (max - min over the repeats).

    python tools/cem_sweep.py [sizes ...] > profiles/cem_sweep.json"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import manytor_amd as m  # noqa: E402

T, K = 12, 7
CANDIDATES = (8, 16, 64)
REPS = 9
SEED = 0x7A9E
LO, HI = -180.0, 180.0


def stats(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4), "spread": round(s[-1] - s[0], 4)}


def moments(eng):
    dev = torch.device("cuda", eng.device)
    g = torch.Generator(device=dev)
    g.manual_seed(SEED)
    mean = torch.empty((T, eng.dof, eng.n_envs), device=dev)
    mean.uniform_(-120.0, 120.0, generator=g)
    mean[:, 1:3, :].mul_(0.4)                     # the example's shaping
    sigma = torch.full_like(mean, 40.0)
    return mean, sigma


def cem_struct(eng, mean, sigma, c, e):
    arg = m.lib.MtCem()
    arg.struct_size, arg.n_steps, arg.n_candidates, arg.n_elites = C.sizeof(m.lib.MtCem), T, c, e
    arg.mean, arg.sigma, arg.ld = mean.data_ptr(), sigma.data_ptr(), eng.n_envs
    arg.lo, arg.hi, arg.seed = LO, HI, SEED
    return arg


def cem_call(eng, mean, sigma, c, e):
    n, dev = eng.n_envs, mean.device
    mean_out, sigma_out = torch.empty_like(mean), torch.empty_like(sigma)
    best = torch.empty(n, dtype=torch.int32, device=dev)
    best_ret = torch.empty(n, device=dev)
    arg = cem_struct(eng, mean, sigma, c, e)
    arg.mean_out, arg.sigma_out, arg.out_ld = mean_out.data_ptr(), sigma_out.data_ptr(), n
    arg.best_out, arg.best_return_out = best.data_ptr(), best_ret.data_ptr()

    def run(_keep=(mean_out, sigma_out, best, best_ret)):
        m.lib.check(eng._lib.mt_cem(eng._h, C.byref(arg)), eng._h)
    return run


def parts_call(eng, mean, sigma, c, e, sampled):
    n, d, dev = eng.n_envs, eng.dof, mean.device
    score = torch.empty((c, n), device=dev)
    best = torch.empty(n, dtype=torch.int32, device=dev)
    best_ret = torch.empty(n, device=dev)
    envs = torch.arange(n, device=dev)
    draw = cem_struct(eng, mean, sigma, c, e)
    g = torch.Generator(device=dev)
    g.manual_seed(SEED)
    sh = m.lib.MtShoot()
    sh.struct_size, sh.n_steps, sh.n_candidates, sh.commit_steps = C.sizeof(m.lib.MtShoot), T, c, 0
    sh.ld, sh.cand_stride = n, T * d * n
    sh.returns_out, sh.ret_ld = score.data_ptr(), n
    sh.best_out, sh.best_return_out = best.data_ptr(), best_ret.data_ptr()

    def run(_keep=(score, best, best_ret)):
        if sampled:
            plans = torch.empty((c, T, d, n), device=dev)
            m.lib.check(eng._lib.mt_sample_plans(eng._h, C.byref(draw), C.c_void_p(plans.data_ptr()), n, T * d * n), eng._h)
        else:
            plans = torch.randn((c, T, d, n), device=dev, generator=g)
            plans.mul_(sigma).add_(mean).clamp_(LO, HI)
        sh.actions = plans.data_ptr()
        m.lib.check(eng._lib.mt_shoot(eng._h, C.byref(sh)), eng._h)
        elites = torch.topk(score, e, dim=0).indices                # (E, N)
        x = plans[elites, :, :, envs]                              # (E, N, T, D): the gather
        mean_out = x.mean(dim=0).permute(1, 2, 0).contiguous()
        sigma_out = x.std(dim=0, unbiased=False).permute(1, 2, 0).contiguous()
        return plans, mean_out, sigma_out
    return run


def timed(eng, fn, episode):
    eng.reset_random(SEED, episode)
    torch.cuda.synchronize(eng.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    keep = fn()
    t1.record()
    t1.synchronize()
    del keep
    return t0.elapsed_time(t1)                    # ms per iteration


def measure(n, table, c):
    e = c // 4
    eng = m.StepEngine(n, K, dh_table=table, radius=51.3 if len(table) == 4 else 92.6, pickup_tol=20.0)
    eng.use_torch_stream()
    mean, sigma = moments(eng)
    paths = {"cem": cem_call(eng, mean, sigma, c, e), "torch": parts_call(eng, mean, sigma, c, e, False),
             "sampled": parts_call(eng, mean, sigma, c, e, True)}
    for fn in paths.values():
        for _ in range(2):
            timed(eng, fn, 0)
    ms = {k: [] for k in paths}
    for r in range(REPS):
        for k, fn in paths.items():
            ms[k].append(timed(eng, fn, r + 1))
    out = {k: stats(v) for k, v in ms.items()}
    a = out["cem"]
    for k in ("torch", "sampled"):
        b = out[k]
        out[f"{k}_over_cem"] = round(b["median"] / a["median"], 3)
        out[f"{k}_separated"] = bool(abs(a["median"] - b["median"]) > max(a["spread"], b["spread"]))
    d = eng.dof
    state = 4 * d + 4 + 12 * K
    # cem    : the state once + mean and sigma read by every candidate's wave and by the refit (cache hits past the first) + the
    #          refit written + best / best_return; DRAM traffic if every re-read hits: state + 8 D T + 8 D T + 8
    # parts  : the draw (randn out; mul, add, clamp: 3 x in and out, mean / sigma in; or sample_plans: mean / sigma in, block out)
    #          + shoot (block in, state, scores and best out) + topk (scores in, indices out) + gather (E plans in and out)
    #          + mean and std (E plans in twice, T D out twice) + two permute copies
    block = 4 * d * T * c
    shoot = block + state + 4 * c + 8
    tail = (4 * c + 8 * e) + 2 * 4 * d * T * e + (2 * 4 * d * T * e + 2 * 4 * d * T) + 4 * 4 * d * T
    out["bytes_per_env"] = {"cem": state + 16 * d * T + 8,
                            "torch": block + 3 * 2 * block + 8 * d * T + shoot + tail,
                            "sampled": 8 * d * T + block + shoot + tail}
    eng.close()
    del mean, sigma, paths
    torch.cuda.empty_cache()
    return out


def main():
    sizes = [int(v) for v in sys.argv[1:]] or [65536, 262144, 1048576]
    res = {"T": T, "K": K, "elites": "C / 4", "reps": REPS, "unit": "device ms per CEM iteration of the whole batch",
           "bytes_per_env_note": "DRAM traffic of one iteration if every re-read of a row hits a cache; a model, not a measurement"}
    for name, table in (("ref4_k7", m.REF_DH_TABLE), ("dh7_k7", m.DH7_TABLE)):
        res[name] = {}
        for n in sizes:
            res[name][str(n)] = {}
            for c in CANDIDATES:
                res[name][str(n)][f"C{c}"] = measure(n, table, c)
                print(f"# {name} n={n} C={c}: {json.dumps(res[name][str(n)][f'C{c}'])}", file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
