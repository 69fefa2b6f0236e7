#!/usr/bin/env python3
"""PPO (clipped surrogate, GAE) on a small MLP policy and an MLP critic without torch autograd anywhere and without a
transposed copy of the logs: every pass over the samples is one engine call on the logs as rollout_policy wrote them.

  1. rollout_policy(sigma=s, actions=True, observations=True, log=True, logp=True, critic=phi's layers): T steps, Gaussian
     exploration in-kernel, and from the SAME launch log pi_old(a | x) and V(x) per sample and the bootstrap V(x_T)
  2. (--collect parts: the four calls that launch replaces, whose results are the same bit for bit -- policy_eval(theta, obs,
     actions=, sigma=s) for log pi_old, values(phi, obs) for V, observe() and values on the resident observation rows, read
     in place as a one-step block, for V(x_T))
  3. gae(reward, done, V, last_value=V(x_T), mask_after_done=True, weights=True): advantages, value targets, and the
     weights that take the steps behind an env's episode end out of both gradients
  4. a few epochs of: policy_grad(adv, old_logp=, clip=, weights=) -- the new log pi, the ratio, the clip decision and the
     gradient in ONE pass over the logs, with the clipped and used counts beside it -- and value_grad(returns, weights); two
     steps of fixed length.  --parts runs the same epoch as the parts that call replaces: policy_eval for the new log pi,
     ratio, clip mask and coef as four elementwise torch lines on (T, N), policy_grad(coef): a second forward pass.

No learning curve is promised: this is the shape of the loop, with the plainest step rule that does not diverge.

    python examples/ppo_train.py --envs 65536 --iterations 20
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
ap.add_argument("--width", type=int, default=32, help="units of the one hidden layer of the policy and of the critic (<= 64)")
ap.add_argument("--iterations", type=int, default=20)
ap.add_argument("--epochs", type=int, default=4)
ap.add_argument("--sigma", type=float, default=15.0, help="exploration noise, degrees")
ap.add_argument("--gamma", type=float, default=0.95)
ap.add_argument("--lam", type=float, default=0.9)
ap.add_argument("--clip", type=float, default=0.2)
ap.add_argument("--lr", type=float, default=0.0003, help="length of the policy's step: theta += lr * grad / |grad|")
ap.add_argument("--value-lr", type=float, default=0.02, help="length of the critic's step")
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--collect", choices=("fused", "parts"), default="fused",
                help="fused: logp, values and the bootstrap value from the rollout's launch; parts: the four calls it replaces")
ap.add_argument("--parts", action="store_true", help="policy_eval + four torch lines + policy_grad instead of the one fused call")
args = ap.parse_args()

eng = m.StepEngine(args.envs, args.targets)
eng.use_torch_stream()
widths = (args.width,)
n_in, dof = 3 * args.targets, eng.dof
gen = torch.Generator(device="cuda").manual_seed(args.seed)


def init(n_out):
    return eng.flatten_policy([
        (torch.randn(args.width, n_in, device="cuda", generator=gen) / (60.0 * n_in ** 0.5), torch.zeros(args.width, device="cuda")),
        (torch.randn(n_out, args.width, device="cuda", generator=gen) * args.width ** -0.5, torch.zeros(n_out, device="cuda"))])


theta, phi = init(dof), init(1)                      # the policy (P floats) and the critic (P_v = value_size(widths) floats)
assert phi.numel() == eng.value_size(widths)
grad, vgrad = torch.empty_like(theta), torch.empty_like(phi)
pi = dict(sigma=args.sigma, widths=widths, out_scale=179.0)

for it in range(args.iterations):
    eng.reset_random(seed=args.seed, episode=it)
    fused = args.collect == "fused"
    ac = dict(logp=True, critic=eng.unflatten_value(phi, widths)) if fused else {}
    log = eng.rollout_policy(eng.unflatten_policy(theta, widths), args.steps, sigma=args.sigma, draw=it, seed=args.seed,
                             out_scale=179.0, log=True, returns=True, actions=True, observations=True, **ac)
    obs, actions = log["observations"], log["actions"]
    if fused:
        old, values, last = log["logp"], log["values"], log["last_value"]
    else:
        old = eng.policy_eval(theta, obs, actions=actions, mean=False, **pi)["logp"]
        values = eng.values(phi, obs, widths=widths)
        eng.observe()                                # x_T: the observation of the state the last step left
        last = eng.values(phi, eng.device_tensor(m.lib.F_OBS)[None], widths=widths)[0]
    est = eng.gae(log["reward"], log["done"], values, last_value=last, gamma=args.gamma, lam=args.lam, mask_after_done=True,
                  weights=True)
    adv, returns, weights = est["advantages"], est["returns"], est["weights"]
    for epoch in range(args.epochs):
        if args.parts:
            new = eng.policy_eval(theta, obs, actions=actions, mean=False, **pi)["logp"]
            ratio = torch.exp(new - old)
            clipped = ((ratio > 1 + args.clip) & (adv > 0)) | ((ratio < 1 - args.clip) & (adv < 0))
            coef = torch.where(clipped, torch.zeros_like(adv), ratio * adv)      # d/dtheta of min(ratio A, clip(ratio) A)
            clip_fraction = clipped.float().sum() / weights.sum()
            eng.policy_grad(theta, obs, actions, coef, scale=1.0 / args.envs, grad_out=grad, **pi)
        else:
            res = eng.policy_grad(theta, obs, actions, adv, old_logp=old, clip=args.clip, weights=weights, scale=1.0 / args.envs,
                                  grad_out=grad, **pi)
            clip_fraction = res["clipped"] / res["used"].clamp_min(1)
        _, vloss = eng.value_grad(phi, obs, returns, weights, widths=widths, scale=1.0 / args.envs, grad_out=vgrad, loss=True)
        theta += (args.lr / grad.norm().clamp_min(1e-20)) * grad
        phi += (args.value_lr / vgrad.norm().clamp_min(1e-20)) * vgrad
    print(f"iteration {it:3d}: mean return over {args.steps} steps {log['returns'].mean().item():+.4f}  "
          f"value loss {-vloss.item():.4e}  clipped {clip_fraction.item():.3f}  |grad| {grad.norm().item():.3e}")
