#!/usr/bin/env python3
"""Training a small MLP policy with an antithetic evolution strategy, one StepEngine.es call per generation.

Each generation
  1. resets the batch so that every member meets the SAME G = envs / members target sets (the G sets tiled over the members):
     members are then compared on common scenes and the fitness differences are the policies', not the scenes'.  That is
     this script's choice, not the call's -- es() scores each member on whatever state its envs are in; and
  2. makes one eng.es(..., inplace=True): the members are drawn around theta, scored over --steps steps on their own envs
     and theta moves along the rank-shaped gradient estimate, all on the device, in four launches.

    python examples/es_train.py --envs 65536 --members 64 --generations 50
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import manytor_amd as m  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--members", type=int, default=64, help="even; envs / members must be a multiple of 256")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--targets", type=int, default=7)
ap.add_argument("--width", type=int, default=32, help="units of the one hidden layer (<= 64)")
ap.add_argument("--generations", type=int, default=50)
ap.add_argument("--sigma", type=float, default=0.02)
ap.add_argument("--lr", type=float, default=0.003, help="step along the rank-shaped estimate, whose entries are of the order of 1 / sigma")
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
assert theta.numel() == eng.policy_size(widths)

# workspaces that live across the generations: no generation allocates them again
population = torch.empty((args.members, theta.numel()), device="cuda")
returns = torch.zeros(args.envs, device="cuda")
G = args.envs // args.members
points = eng.device_tensor(m.lib.F_POINTS)          # (3K, N) view of the resident targets

for g in range(args.generations):
    eng.reset_random(seed=args.seed, episode=g)     # fresh targets for everybody ...
    scenes = points[:, :G].T.reshape(G, args.targets, 3)                    # member 0's, env-major (G, K, 3) ...
    eng.reset(scenes.repeat(args.members, 1, 1).contiguous())               # ... tiled over the members
    res = eng.es(theta, args.sigma, members=args.members, steps=args.steps, widths=widths, lr=args.lr, inplace=True, draw=g,
                 seed=args.seed, out_scale=179.0, population=population, returns=returns)
    fit = res["fitness"]
    print(f"generation {g:3d}: mean fitness {fit.mean().item():+.3f}  best {fit.max().item():+.3f} (member {int(res['best'])})  "
          f"|grad| {res['grad'].norm().item():.3e}")

final = eng.unflatten_policy(theta, widths)         # [(weight, bias), ...] views: rollout_policy takes them as they are
eng.reset_random(seed=args.seed + 1, episode=0)
ret = eng.rollout_policy(final, args.steps, out_scale=179.0, returns=True)["returns"]
print(f"theta after {args.generations} generations on unseen targets: mean return over {args.steps} steps {ret.mean().item():+.3f}")
