#!/usr/bin/env python3
"""A scripted expert: every step, each arm solves for the joint angles that carry its pickup frame to its nearest alive
target (ik(stage=True): damped least squares, one launch) and executes them (step(): one launch).  Two launches per
env-step, no sampling, no learning.

  1. episodes x steps of (ik(stage=True); step(); reset_done()): an arm that cleared its table starts its next episode at
     once; the mean return per arm and `steps` steps is printed beside the same loop on sample_actions (the reference's
     random agent, test_multi.py:19-21)
  2. --clone: the expert's (observation, IK angles) pairs are logged and an MLP is fitted to them with
     policy_grad(coef=ones, sigma=1) -- behaviour cloning without autograd -- and then run in the loop itself

No learning curve is promised, and the ground rule (-1 when the route dips below z = 0) is not the solver's concern: the
printed return is what it is.

    python examples/expert_reach.py --envs 65536 --episodes 5 --clone
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
ap.add_argument("--episodes", type=int, default=5)
ap.add_argument("--iters", type=int, default=16, help="solver iterations per step")
ap.add_argument("--clone", action="store_true", help="fit an MLP to the expert's actions and run it")
ap.add_argument("--width", type=int, default=64)
ap.add_argument("--epochs", type=int, default=200)
ap.add_argument("--lr", type=float, default=0.05, help="length of a cloning step: theta += lr * grad / |grad|")
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()

eng = m.StepEngine(args.envs, args.targets)
eng.use_torch_stream()
n, dof, n_in = args.envs, eng.dof, 3 * args.targets
obs_rows = eng.device_tensor(m.lib.F_OBS)
reward_row = eng.device_tensor(m.lib.F_REWARD)


def episodes(act, log=None):
    """Mean return per arm and episode length of `act` (a function that stages the next actions) over args.episodes x
    args.steps steps, finished arms re-armed by reset_done after every step; log: (obs, angles) blocks of the first
    args.steps steps to fill."""
    eng.reset_random(args.seed, 0)
    total = torch.zeros((), device="cuda")
    for t in range(args.episodes * args.steps):
        logging = log is not None and t < args.steps
        if logging:
            eng.observe()                                        # the policy's input: the observation the step starts from
            log[0][t].copy_(obs_rows)
        angles = act(t)
        if logging:
            log[1][t].copy_(angles)
        eng.step()
        total += reward_row.float().mean()
        eng.reset_done(args.seed)
    return float(total) / args.episodes


def expert(_):
    return eng.ik(stage=True, iters=args.iters, residual=False, index=False)["angles"]


def random_agent(step):
    eng.sample_actions(args.seed, step)
    return None


log = (torch.empty((args.steps, n_in, n), device="cuda"), torch.empty((args.steps, dof, n), device="cuda")) if args.clone else None
print(f"expert (ik + step): mean return per arm and episode {episodes(expert, log):+.3f}")
print(f"random actions     : mean return per arm and episode {episodes(random_agent):+.3f}")

if args.clone:
    gen = torch.Generator(device="cuda").manual_seed(args.seed)
    widths = (args.width,)
    theta = eng.flatten_policy([
        (torch.randn(args.width, n_in, device="cuda", generator=gen) / (60.0 * n_in ** 0.5), torch.zeros(args.width, device="cuda")),
        (torch.randn(dof, args.width, device="cuda", generator=gen) * args.width ** -0.5, torch.zeros(dof, device="cuda"))])
    obs, angles = log
    ones = torch.ones((args.steps, n), device="cuda")
    grad = torch.empty_like(theta)
    for epoch in range(args.epochs):
        _, loss = eng.policy_grad(theta, obs, angles, ones, sigma=1.0, widths=widths, out_scale=180.0, scale=1.0 / (args.steps * n),
                                  grad_out=grad, loss=True)
        theta.add_(grad, alpha=args.lr / float(grad.norm().clamp_min(1e-12)))
        if epoch % 50 == 0 or epoch == args.epochs - 1:
            print(f"clone epoch {epoch:4d}: mean squared error {-2.0 * float(loss) / dof:10.2f} deg^2 per joint")
    layers = eng.unflatten_policy(theta, widths)

    def cloned(_):
        eng.observe()
        h = torch.tanh(layers[0][0] @ obs_rows + layers[0][1][:, None])
        a = 180.0 * torch.tanh(layers[1][0] @ h + layers[1][1][:, None])
        eng.device_tensor(m.lib.F_ACTIONS).copy_(a)
        return a

    print(f"cloned policy      : mean return per arm and episode {episodes(cloned):+.3f}")
