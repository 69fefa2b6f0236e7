#!/usr/bin/env python3
"""MPPI (model-predictive path integral) planning on the engine: every decision runs I iterations of "draw C plans per arm
around (mean, sigma), score them, move the mean to the average of ALL candidates weighted by exp((return - best return) /
lambda)", and the last iteration commits the first H steps of each arm's best plan.  Between decisions the mean is shifted
by H steps (the tail starts from zero).  sigma stays fixed unless --fit-sigma refits it as the weighted deviation (it is
then reset between decisions).  Nothing crosses PCIe; torch and the engine share one stream.

  --mode fused (default): an iteration is ONE call, `eng.mppi(mean, sigma, ..., inplace=True)`: the candidates are drawn in
      the kernel, so no (C, T, D, N) block exists; the weights and the refit are computed where the data sits.
  --mode parts: the same iteration from its parts -- `eng.sample_plans` writes the block, `eng.shoot(all_returns=True)`
      scores it, torch builds the table of powers by the recurrence W[k] = W[k-1] * decay, looks the weights up by the
      integer gap to the best return, and sums weights and weighted plans in ascending candidate order as the kernel does;
      `rollout_actions` commits.
Both modes print the same figures for equal arguments.

    python examples/plan_mppi.py --envs 65536 --candidates 16 --temperature 1.5 --horizon 12 --commit 4 --iterations 3 --decisions 10
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import manytor_amd as m  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--targets", type=int, default=7)
ap.add_argument("--candidates", type=int, default=16)
ap.add_argument("--temperature", type=float, default=1.5)
ap.add_argument("--horizon", type=int, default=12)
ap.add_argument("--commit", type=int, default=4)
ap.add_argument("--iterations", type=int, default=3)
ap.add_argument("--decisions", type=int, default=10)
ap.add_argument("--sigma", type=float, default=60.0)
ap.add_argument("--sigma-min", type=float, default=2.0)
ap.add_argument("--fit-sigma", action="store_true")
ap.add_argument("--pickup-tol", type=float, default=20.0)
ap.add_argument("--mode", choices=("fused", "parts"), default="fused")
args = ap.parse_args()
N, C, T, H, I = args.envs, args.candidates, args.horizon, min(args.commit, args.horizon), args.iterations
decay = float(np.float32(np.exp(-1.0 / args.temperature)))      # what eng.mppi(temperature=) hands to the library

eng = m.StepEngine(N, args.targets, pickup_tol=args.pickup_tol, return_ring=4)
eng.use_torch_stream()
eng.reset_random(seed=1, episode=0)
D = eng.dof
dev = torch.device("cuda", eng.device)
mean = torch.zeros((T, D, N), device=dev)
sigma = torch.full((T, D, N), args.sigma, device=dev)
sigma[:, 1:3].mul_(0.4)                          # shoulder and elbow kept near the upper half: most plans stay above ground
sigma0 = sigma.clone()
earned = torch.zeros(N, device=dev)
cols = torch.arange(N, device=dev)
table = torch.ones(2 * T + 1, device=dev)        # W[0] = 1, W[k] = W[k-1] * decay: one fp32 rounding per entry
rho = torch.tensor(decay, device=dev)
for k in range(1, 2 * T + 1):
    table[k] = table[k - 1] * rho
predicted = None


def iteration_from_parts(draw, commit):
    """What eng.mppi(mean, sigma, inplace=True, ...) does, from calls the engine had before it."""
    plans = eng.sample_plans(mean, sigma, candidates=C, draw=draw, seed=1, keep_mean=True)
    out = eng.shoot(plans, all_returns=True)
    w = table[(out["best_return"] - out["candidate_returns"]).long()]                  # (C, N)
    total = torch.zeros(N, device=dev)
    acc = torch.zeros((T, D, N), device=dev)
    for c in range(C):
        total += w[c]
        acc += w[c] * plans[c]
    mu = acc / total
    if args.fit_sigma:
        var = torch.zeros((T, D, N), device=dev)
        for c in range(C):
            d = plans[c] - mu
            var += w[c] * (d * d)
        sigma.copy_(torch.clamp_min(torch.sqrt(var / total), args.sigma_min))
    mean.copy_(mu)
    res = {"best_return": out["best_return"], "weight_sum": total}
    if commit:
        chosen = plans[out["best"].long(), :commit, :, cols].permute(1, 2, 0).contiguous()
        res["returns"] = eng.rollout_actions(chosen, layout="soa", auto_reset=True, seed=1, returns=True)["returns"]
    return res


t0 = time.perf_counter()
for dec in range(args.decisions):
    for it in range(I):
        commit = H if it == I - 1 else 0
        draw = dec * I + it
        if args.mode == "fused":
            res = eng.mppi(mean, sigma, candidates=C, temperature=args.temperature, draw=draw, seed=1, commit=commit,
                           auto_reset=commit > 0, sigma_min=args.sigma_min, keep_mean=True, fit_sigma=args.fit_sigma,
                           inplace=True, returns=True)
        else:
            res = iteration_from_parts(draw, commit)
        if commit:
            earned += res["returns"]
    predicted, effective = res["best_return"], res["weight_sum"]
    if H:
        mean[:T - H] = mean[H:].clone()
        mean[T - H:] = 0.0
    if args.fit_sigma:
        sigma.copy_(sigma0)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
steps = args.decisions * (I * C * T + H) * N
print(f"[{args.mode}] {N} arms, {args.decisions} decisions of {I} MPPI iterations ({C} candidates, lambda {args.temperature:g}, "
      f"{T} steps) + {H} committed steps: {dt * 1e3:.1f} ms, {steps / dt:.3g} env-steps/s evaluated; mean reward earned per arm "
      f"{earned.mean().item():+.4f} (best plan's predicted return, last decision: {predicted.mean().item():+.4f}; sum of "
      f"weights {effective.mean().item():.4f}); episodes finished per arm {eng.finished().mean():.4f}; "
      f"refused actions {eng.bad_action_count()}")
eng.close()
