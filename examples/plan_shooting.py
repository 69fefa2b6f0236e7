#!/usr/bin/env python3
"""Random shooting on the engine: score a few candidate action tapes per arm WITHOUT committing the state, then commit
the first chunk of the best one.

Every planning round draws C candidate plans of T steps for all N arms on the device -- a (T, D, N) block of angles
each -- and asks "what would these T actions earn from here?".  Each arm then keeps the candidate with the best return,
and the first `--commit` steps of that plan are executed for real (auto_reset re-arms an arm that picks up its last
target).  Nothing crosses PCIe; torch and the engine share one stream.

  --mode fused (default): the whole round is ONE call, `eng.shoot(plans, commit=H, auto_reset=True)`: the engine scores
      all candidates of an arm from one read of its state, picks the best on the device and commits its first H steps.
  --mode launches: the same round from its parts -- one `rollout_actions(..., dry_run=True, returns=True)` launch per
      candidate, a torch argmax, a torch gather of the chosen plans and the committing launch.
Both modes print the same rewards and episode counts for equal arguments.

    python examples/plan_shooting.py --envs 65536 --candidates 8 --horizon 12 --commit 4 --rounds 10
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
ap.add_argument("--candidates", type=int, default=8)
ap.add_argument("--horizon", type=int, default=12)
ap.add_argument("--commit", type=int, default=4)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--pickup-tol", type=float, default=20.0)
ap.add_argument("--mode", choices=("fused", "launches"), default="fused")
args = ap.parse_args()
N, C, T, H = args.envs, args.candidates, args.horizon, min(args.commit, args.horizon)

eng = m.StepEngine(N, args.targets, pickup_tol=args.pickup_tol, return_ring=4)
eng.use_torch_stream()                          # tapes are written by torch ops right ahead of the calls that read them
eng.reset_random(seed=1, episode=0)
D = eng.dof
dev = torch.device("cuda", eng.device)
gen = torch.Generator(device=dev)
gen.manual_seed(7)
plans = torch.empty((C, T, D, N), device=dev)    # candidate c = plans[c]: the (T, D, N) layout the kernel reads in place
score = torch.empty((C, N), device=dev)
earned = torch.zeros(N, device=dev)

t0 = time.perf_counter()
for rnd in range(args.rounds):
    # shoulder and elbow kept in the upper half so that most plans stay above ground; the rest uniform
    plans.uniform_(-180.0, 180.0, generator=gen)
    plans[:, :, 1:3, :].mul_(0.4)
    if args.mode == "fused":
        last = rnd == args.rounds - 1                                            # (the scores are only printed)
        out = eng.shoot(plans, commit=H, auto_reset=H > 0, seed=1, returns=True, all_returns=last)
        if last:
            score = out["candidate_returns"]
        if H > 0:
            earned += out["returns"]
        continue
    for c in range(C):
        score[c] = eng.rollout_actions(plans[c], layout="soa", dry_run=True, returns=True)["returns"]
    best = score.argmax(dim=0)                                               # (N,) index of each arm's best plan
    chosen = plans[best, :H, :, torch.arange(N, device=dev)]                 # (N, H, D)
    out = eng.rollout_actions(chosen.permute(1, 0, 2), layout="env_major", auto_reset=True, seed=1, returns=True)
    earned += out["returns"]
torch.cuda.synchronize()
dt = time.perf_counter() - t0
steps = args.rounds * (C * T + H) * N
print(f"[{args.mode}] {N} arms, {args.rounds} rounds of {C} x {T}-step dry runs + {H} committed steps: {dt * 1e3:.1f} ms, "
      f"{steps / dt:.3g} env-steps/s evaluated; mean reward earned per arm {earned.mean().item():+.3f} "
      f"(best plan's predicted return, last round: {score.max(dim=0).values.mean().item():+.3f}; "
      f"a random plan's: {score.mean().item():+.3f}); episodes finished per arm {eng.finished().mean():.3f}; "
      f"refused actions {eng.bad_action_count()}")
eng.close()
