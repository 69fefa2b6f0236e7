#!/usr/bin/env python3
"""An MLP policy in the loop, two ways.

    --mode fused   one StepEngine.rollout_policy call per chunk of T steps: observation, MLP and step run T times inside ONE
                   launch, the state stays in registers / LDS, and only what is asked for (here: the returns) is written
    --mode parts   the loop of examples/policy_loop.py: observe() -> torch MLP on the zero-copy views -> step(), one round
                   of launches per step

Both modes run the same weights (two hidden tanh layers, a tanh output scaled to +-179 degrees) from the same reset, so
they take the same actions up to the rounding of the MLP, and print the same kind of figures.

    python examples/policy_rollout.py --envs 1048576 --steps 200 --mode fused
    python examples/policy_rollout.py --envs 1048576 --steps 200 --mode parts
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import manytor_amd as m  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=1 << 20)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--targets", type=int, default=7)
ap.add_argument("--width", type=int, default=32, help="units of each of the two hidden layers (<= 64)")
ap.add_argument("--chunk", type=int, default=20, help="fused mode: steps per rollout_policy call")
ap.add_argument("--mode", choices=("fused", "parts"), default="fused")
args = ap.parse_args()

eng = m.StepEngine(args.envs, args.targets)
eng.use_torch_stream()
eng.reset_random(seed=1, episode=0)

n_in, dof = 3 * args.targets, eng.dof
gen = torch.Generator(device="cuda").manual_seed(7)
sizes = [n_in, args.width, args.width, dof]
layers = [(torch.randn(o, i, device="cuda", generator=gen) * (1.0 / (60.0 * n_in ** 0.5) if l == 0 else i ** -0.5),
           torch.randn(o, device="cuda", generator=gen) * 0.1) for l, (i, o) in enumerate(zip(sizes[:-1], sizes[1:]))]
ret = eng.device_tensor(m.lib.F_TOTAL_REWARD)   # (N,)

if args.mode == "fused":
    def run(steps):
        for s in range(0, steps, args.chunk):
            eng.rollout_policy(layers, min(args.chunk, steps - s), hidden="tanh", out="tanh", out_scale=179.0)
else:
    obs = eng.device_tensor(m.lib.F_OBS)        # (3K, N) view of the observation rows
    act = eng.device_tensor(m.lib.F_ACTIONS)    # (D, N)  view of the staging buffer mt_step reads

    def run(steps):
        for _ in range(steps):
            eng.observe()                       # the observation of the state the step starts from
            h = obs
            for w, b in layers[:-1]:
                h = torch.tanh(torch.addmm(b[:, None], w, h))
            w, b = layers[-1]
            torch.tanh(torch.addmm(b[:, None], w, h), out=act).mul_(179.0)
            eng.step()

run(min(5, args.steps))
torch.cuda.synchronize()
t0 = time.perf_counter()
run(args.steps)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f"{args.envs} arms x {args.steps} steps with a 2x{args.width} MLP policy in the loop ({args.mode}): "
      f"{args.envs * args.steps / dt:.3e} env-steps/s ({dt / args.steps * 1e6:.1f} us per step incl. the policy); "
      f"mean return {ret.mean().item():.2f}")
