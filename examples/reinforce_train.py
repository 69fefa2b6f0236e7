#!/usr/bin/env python3
"""REINFORCE on a small MLP policy without torch autograd anywhere: per iteration one noisy rollout_policy call that logs
what it saw and did, one reward_to_go over the logged rewards, one policy_grad that turns the logs into the flat gradient of
the weighted log-likelihood, and a step of fixed length along it as a torch op.

  1. rollout_policy(sigma=s, actions=True, observations=True, log=True): T steps, the policy's Gaussian exploration in-kernel
  2. reward_to_go(reward, done, gamma, baseline, mask_after_done=True): the sample weights; steps behind an env's episode
     end get 0 and drop out of the gradient
  3. policy_grad(theta, obs, actions, coef, sigma=s, scale=1 / N): grad of mean_i sum_t coef * log pi(a | x)
  4. theta += lr * grad / |grad|

    python examples/reinforce_train.py --envs 65536 --iterations 50
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import manytor_amd as m  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--targets", type=int, default=7)
ap.add_argument("--width", type=int, default=32, help="units of the one hidden layer (<= 64)")
ap.add_argument("--iterations", type=int, default=50)
ap.add_argument("--sigma", type=float, default=15.0, help="exploration noise, degrees")
ap.add_argument("--gamma", type=float, default=0.95)
ap.add_argument("--lr", type=float, default=0.01, help="length of the step in parameter space: theta += lr * grad / |grad|")
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()

eng = m.StepEngine(args.envs, args.targets)
eng.use_torch_stream()
widths = (args.width,)
n_in, dof = 3 * args.targets, eng.dof
gen = torch.Generator(device="cuda").manual_seed(args.seed)
layers = [(torch.randn(args.width, n_in, device="cuda", generator=gen) / (60.0 * n_in ** 0.5), torch.zeros(args.width, device="cuda")),
          (torch.randn(dof, args.width, device="cuda", generator=gen) * args.width ** -0.5, torch.zeros(dof, device="cuda"))]
theta = eng.flatten_policy(layers)
grad = torch.empty_like(theta)
coef = torch.empty((args.steps, args.envs), device="cuda")
baseline = 0.0

for it in range(args.iterations):
    eng.reset_random(seed=args.seed, episode=it)
    log = eng.rollout_policy(eng.unflatten_policy(theta, widths), args.steps, sigma=args.sigma, draw=it, seed=args.seed,
                             out_scale=179.0, log=True, returns=True, actions=True, observations=True)
    eng.reward_to_go(log["reward"], log["done"], args.gamma, baseline, mask_after_done=True, out=coef)
    eng.policy_grad(theta, log["observations"], log["actions"], coef, sigma=args.sigma, widths=widths, out_scale=179.0,
                    scale=1.0 / args.envs, grad_out=grad)
    # the raw gradient spans orders of magnitude between the layers' scales (x is in centimetres and degrees, the output in
    # degrees): a step of fixed length along it, the plainest thing that does not diverge
    theta += (args.lr / grad.norm().clamp_min(1e-20)) * grad
    ret = log["returns"].mean().item()
    baseline = ret / args.steps        # a constant baseline near the mean reward-to-go of the last batch
    print(f"iteration {it:3d}: mean return over {args.steps} steps {ret:+.4f}  |grad| {grad.norm().item():.3e}")
