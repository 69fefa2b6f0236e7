#!/usr/bin/env python3
"""mt_mppi against the calls it replaces and against mt_cem: device time of ONE MPPI iteration -- draw C candidate plans of
T = 12 steps per arm around (mean, sigma), score them, weigh every candidate by decay ** (best return - its return), refit
the mean (and, in the `_sigma` rows, sigma) as the weighted moments -- at 65 536 / 1 048 576 arms, C = 16 and 64, for the
reference arm (D = 4, K = 7) and the 7-joint table.  No commit: the committing launch is the same on every side.

Per point, on ONE handle running on torch's stream, interleaved, REPS repeats after a warm-up, timed between two HIP events
on that stream (tools/cem_sweep.py's protocol):
  mppi / mppi_sigma   : one mt_mppi through the C entry point (refit out of place), outputs allocated outside the region
  parts / parts_sigma : what the library offered before -- mt_sample_plans writes the (C, T, D, N) block, mt_shoot with
                        returns_out scores it, torch turns the scores into weights (exp), sums them, and reduces the block
                        with them (einsum: the block is read once for the mean; the variance needs (x - m)^2, a second
                        block, and a third pass)
  cem                 : one mt_cem at E = C / 4 on the same point (mean and sigma refitted)
Every timed region starts from a freshly reset, idle handle.  A point counts as faster / slower only if the medians differ
by more than the larger spread (max - min over the repeats).

    python tools/mppi_sweep.py [sizes ...] > profiles/mppi_sweep.json"""
import ctypes as C
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import manytor_amd as m  # noqa: E402

T, K = 12, 7
CANDIDATES = (16, 64)
REPS = 9
SEED = 0x7A9E
LO, HI = -180.0, 180.0
LAMBDA = 1.5
DECAY = math.exp(-1.0 / LAMBDA)


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


def mppi_call(eng, mean, sigma, c, fit_sigma):
    n, dev = eng.n_envs, mean.device
    mean_out = torch.empty_like(mean)
    sigma_out = torch.empty_like(sigma) if fit_sigma else None
    best = torch.empty(n, dtype=torch.int32, device=dev)
    best_ret, wsum = torch.empty(n, device=dev), torch.empty(n, device=dev)
    arg = m.lib.MtMppi()
    arg.struct_size, arg.n_steps, arg.n_candidates, arg.decay = C.sizeof(m.lib.MtMppi), T, c, DECAY
    arg.mean, arg.sigma, arg.ld = mean.data_ptr(), sigma.data_ptr(), n
    arg.lo, arg.hi, arg.seed = LO, HI, SEED
    arg.mean_out, arg.out_ld = mean_out.data_ptr(), n
    arg.sigma_out = sigma_out.data_ptr() if fit_sigma else None
    arg.best_out, arg.best_return_out, arg.weight_sum_out = best.data_ptr(), best_ret.data_ptr(), wsum.data_ptr()

    def run(_keep=(mean_out, sigma_out, best, best_ret, wsum)):
        m.lib.check(eng._lib.mt_mppi(eng._h, C.byref(arg)), eng._h)
    return run


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


def parts_call(eng, mean, sigma, c, fit_sigma):
    n, d, dev = eng.n_envs, eng.dof, mean.device
    score = torch.empty((c, n), device=dev)
    best = torch.empty(n, dtype=torch.int32, device=dev)
    best_ret = torch.empty(n, device=dev)
    draw = cem_struct(eng, mean, sigma, c, 1)
    sh = m.lib.MtShoot()
    sh.struct_size, sh.n_steps, sh.n_candidates, sh.commit_steps = C.sizeof(m.lib.MtShoot), T, c, 0
    sh.ld, sh.cand_stride = n, T * d * n
    sh.returns_out, sh.ret_ld = score.data_ptr(), n
    sh.best_out, sh.best_return_out = best.data_ptr(), best_ret.data_ptr()

    def run(_keep=(score, best, best_ret)):
        plans = torch.empty((c, T, d, n), device=dev)
        m.lib.check(eng._lib.mt_sample_plans(eng._h, C.byref(draw), C.c_void_p(plans.data_ptr()), n, T * d * n), eng._h)
        sh.actions = plans.data_ptr()
        m.lib.check(eng._lib.mt_shoot(eng._h, C.byref(sh)), eng._h)
        w = torch.exp((score - best_ret) * (1.0 / LAMBDA))         # (C, N)
        s = w.sum(dim=0)
        mean_out = torch.einsum("cn,ctdn->tdn", w, plans) / s
        sigma_out = None
        if fit_sigma:
            dev2 = (plans - mean_out) ** 2
            sigma_out = torch.sqrt(torch.einsum("cn,ctdn->tdn", w, dev2) / s)
        return plans, mean_out, sigma_out, s
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
    paths = {"mppi": mppi_call(eng, mean, sigma, c, False), "mppi_sigma": mppi_call(eng, mean, sigma, c, True),
             "parts": parts_call(eng, mean, sigma, c, False), "parts_sigma": parts_call(eng, mean, sigma, c, True),
             "cem": cem_call(eng, mean, sigma, c, e)}
    for fn in paths.values():
        for _ in range(2):
            timed(eng, fn, 0)
    ms = {k: [] for k in paths}
    for r in range(REPS):
        for k, fn in paths.items():
            ms[k].append(timed(eng, fn, r + 1))
    out = {k: stats(v) for k, v in ms.items()}
    for ours, theirs in (("mppi", "parts"), ("mppi_sigma", "parts_sigma"), ("mppi_sigma", "cem")):
        a, b = out[ours], out[theirs]
        out[f"{theirs}_over_{ours}"] = round(b["median"] / a["median"], 3)
        out[f"{theirs}_vs_{ours}_separated"] = bool(abs(a["median"] - b["median"]) > max(a["spread"], b["spread"]))
    d = eng.dof
    state = 4 * d + 4 + 12 * K
    block = 4 * d * T * c
    blocks = 2 if d > 4 else 1                    # Philox blocks per plan step
    # mppi   : the state once + mean and sigma read by every candidate's wave and by the refit (cache hits past the first) + the
    #          refit written + best / best_return / weight_sum; DRAM traffic if every re-read hits
    # parts  : sample_plans (mean / sigma in, block out) + shoot (block in, state, scores and best out) + weights (scores in
    #          and out) + the weighted mean (block in, T D out) [+ the deviations (block in and out) + their reduction (block in)]
    shoot = block + state + 4 * c + 8
    out["bytes_per_env"] = {"mppi": state + 12 * d * T + 12, "mppi_sigma": state + 16 * d * T + 12,
                            "parts": 8 * d * T + block + shoot + 8 * c + block + 4 * d * T,
                            "parts_sigma": 8 * d * T + block + shoot + 8 * c + block + 4 * d * T + 3 * block + 4 * d * T}
    # plan steps regenerated from Philox per (arm, step) by the refit, scoring aside: C (2 C with sigma_out) against mt_cem's 2 E
    out["refit_philox_blocks_per_arm_step"] = {"mppi": c * blocks, "mppi_sigma": 2 * c * blocks, "cem": 2 * e * blocks}
    eng.close()
    del mean, sigma, paths
    torch.cuda.empty_cache()
    return out


def main():
    sizes = [int(v) for v in sys.argv[1:]] or [65536, 1048576]
    res = {"T": T, "K": K, "lambda": LAMBDA, "cem_elites": "C / 4", "reps": REPS,
           "unit": "device ms per iteration of the whole batch",
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
