#!/usr/bin/env python3
"""Cross-entropy-method planning on the engine: every decision runs I iterations of "draw C plans per arm around
(mean, sigma), score them, refit (mean, sigma) from the E best", and the last iteration commits the first H steps of each
arm's best plan.  Between decisions the mean is shifted by H steps (the tail starts from zero) and sigma is reset.
Nothing crosses PCIe; torch and the engine share one stream.

  --mode fused (default): an iteration is ONE call, `eng.cem(mean, sigma, ..., inplace=True)`: the candidates are drawn in
      the kernel, so no (C, T, D, N) block exists; the elites are picked and (mean, sigma) refitted where the data sits.
  --mode parts: the same iteration from its parts -- `eng.sample_plans` writes the block, `eng.shoot(all_returns=True)`
      scores it, a stable torch sort picks the elites (return descending, index ascending), a torch gather collects their
      plans, the refit sums them in ascending index order as the kernel does, and `rollout_actions` commits.
Both modes print the same figures for equal arguments.

    python examples/plan_cem.py --envs 65536 --candidates 16 --elites 4 --horizon 12 --commit 4 --iterations 3 --decisions 10
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import manytor_amd as m  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--targets", type=int, default=7)
ap.add_argument("--candidates", type=int, default=16)
ap.add_argument("--elites", type=int, default=4)
ap.add_argument("--horizon", type=int, default=12)
ap.add_argument("--commit", type=int, default=4)
ap.add_argument("--iterations", type=int, default=3)
ap.add_argument("--decisions", type=int, default=10)
ap.add_argument("--sigma", type=float, default=60.0)
ap.add_argument("--sigma-min", type=float, default=2.0)
ap.add_argument("--pickup-tol", type=float, default=20.0)
ap.add_argument("--mode", choices=("fused", "parts"), default="fused")
args = ap.parse_args()
N, C, E, T, H, I = args.envs, args.candidates, args.elites, args.horizon, min(args.commit, args.horizon), args.iterations

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
inv_e = torch.tensor(1.0, device=dev) / E        # the fp32 nearest to 1 / E
predicted = None


def iteration_from_parts(draw, commit):
    """What eng.cem(mean, sigma, inplace=True, ...) does, from calls the engine had before it."""
    plans = eng.sample_plans(mean, sigma, candidates=C, draw=draw, seed=1, keep_mean=True)
    out = eng.shoot(plans, all_returns=True)
    order = torch.sort(-out["candidate_returns"], dim=0, stable=True).indices[:E]      # return descending, index ascending
    elites = torch.sort(order, dim=0).values                                           # (E, N), ascending
    x = [plans[elites[k], :, :, cols].permute(1, 2, 0) for k in range(E)]              # E x (T, D, N)
    mu = x[0].clone()
    for k in range(1, E):
        mu += x[k]
    mu *= inv_e
    var = (x[0] - mu) ** 2
    for k in range(1, E):
        var += (x[k] - mu) ** 2
    var *= inv_e
    mean.copy_(mu)
    sigma.copy_(torch.clamp_min(torch.sqrt(var), args.sigma_min))
    res = {"best_return": out["best_return"]}
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
            res = eng.cem(mean, sigma, candidates=C, elites=E, draw=draw, seed=1, commit=commit, auto_reset=commit > 0,
                          sigma_min=args.sigma_min, keep_mean=True, inplace=True, returns=True)
        else:
            res = iteration_from_parts(draw, commit)
        if commit:
            earned += res["returns"]
    predicted = res["best_return"]
    if H:
        mean[:T - H] = mean[H:].clone()
        mean[T - H:] = 0.0
    sigma.copy_(sigma0)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
steps = args.decisions * (I * C * T + H) * N
print(f"[{args.mode}] {N} arms, {args.decisions} decisions of {I} CEM iterations ({C} candidates, {E} elites, {T} steps) + {H} "
      f"committed steps: {dt * 1e3:.1f} ms, {steps / dt:.3g} env-steps/s evaluated; mean reward earned per arm "
      f"{earned.mean().item():+.4f} (best plan's predicted return, last decision: {predicted.mean().item():+.4f}); "
      f"episodes finished per arm {eng.finished().mean():.4f}; refused actions {eng.bad_action_count()}")
eng.close()
