#!/usr/bin/env python3
"""mt_ppo_grad against the parts it replaces in a PPO epoch, and mt_policy_grad alone (which the PPO mode must not have
slowed down): device time over the logs of T = 20 steps at 65 536 / 1 048 576 arms of the reference arm (D = 4, K = 7), for
the policies of tools/policy_grad_sweep.py, (L, width) = (1, -), (2, 32), (3, 32), (3, 64).

Per point, on ONE handle running on torch's stream, interleaved, REPS repeats after a warm-up, timed between two HIP events
on that stream (tools/policy_rollout_sweep.py's protocol):
  fused        one policy_grad(adv, old_logp=, clip=, weights=): mt_ppo_grad, two launches
  parts        policy_eval(mean=False) for the new logp; ratio, clip mask, coef and the clip fraction as the four torch lines of
               examples/ppo_train.py --parts; policy_grad(coef): a second forward pass and about eight elementwise launches
  policy_grad  mt_policy_grad alone, with the advantages as its coef (the same call on this commit and on the parent)
old_logp is the logp under weights moved by 2 % so that both clip classes are populated (the clip fraction is recorded).
A point counts as faster / slower only if the medians differ by more than the larger spread (max - min over the repeats).

    python tools/ppo_grad_sweep.py [sizes ...] > profiles/ppo_grad_sweep.json
    python tools/ppo_grad_sweep.py --policy-grad-only --root PARENT_CHECKOUT [sizes ...]     # the parent's mt_policy_grad

With --merge-parent FILE the output of the second command is attached to the first as `parent_policy_grad` per point."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="*", type=int)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the built tree whose manytor_amd is measured (default: this one)")
ap.add_argument("--policy-grad-only", action="store_true", help="time mt_policy_grad alone (all a parent checkout has)")
ap.add_argument("--merge-parent", default=None, help="a --policy-grad-only result of the parent commit to record beside this one")
args = ap.parse_args()

import torch  # noqa: E402

sys.path.insert(0, args.root)
import manytor_amd as m  # noqa: E402

T, K = 20, 7
POLICIES = ((1, 0), (2, 32), (3, 32), (3, 64))
REPS = 9
SEED = 0x7A9E
OUT_SCALE = 179.0
SIGMA = 15.0
CLIP = 0.2


def stats(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4), "spread": round(s[-1] - s[0], 4)}


def make_layers(eng, n_layers, width):
    dev = torch.device("cuda", eng.device)
    g = torch.Generator(device=dev)
    g.manual_seed(SEED)
    n_in = 3 * K
    sizes = [n_in] + [width] * (n_layers - 1) + [eng.dof]
    return [(torch.randn(o, i, device=dev, generator=g) * (1.0 / (60.0 * n_in ** 0.5) if l == 0 else i ** -0.5),
             torch.randn(o, device=dev, generator=g) * 0.1) for l, (i, o) in enumerate(zip(sizes[:-1], sizes[1:]))]


def timed(eng, fn):
    torch.cuda.synchronize(eng.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)          # ms per pass over the whole batch


def measure(n, n_layers, width):
    eng = m.StepEngine(n, K)
    eng.use_torch_stream()
    eng.reset_random(SEED, 0)
    layers = make_layers(eng, n_layers, width)
    pi = dict(sigma=SIGMA, out_scale=OUT_SCALE)
    log = eng.rollout_policy(layers, T, sigma=SIGMA, seed=SEED, out_scale=OUT_SCALE, log=True, actions=True, observations=True)
    obs, actions = log["observations"], log["actions"]
    adv = eng.reward_to_go(log["reward"], log["done"], 0.95, 0.0, mask_after_done=True)
    adv = adv - adv.mean()
    weights = torch.ones_like(adv)
    grad = torch.zeros(eng.policy_size((width,) * (n_layers - 1)), device=adv.device)
    paths, out = {}, {}
    if not args.policy_grad_only:
        g = torch.Generator(device=adv.device)
        g.manual_seed(SEED + 1)
        moved = [(w * (1 + 0.02 * torch.randn(w.shape, device=w.device, generator=g)), b) for w, b in layers]
        old = eng.policy_eval(moved, obs, actions=actions, mean=False, **pi)["logp"]
        state = {}

        def fused():
            state["res"] = eng.policy_grad(layers, obs, actions, adv, old_logp=old, clip=CLIP, weights=weights, scale=1.0 / n,
                                           grad_out=grad, **pi)

        def parts():
            new = eng.policy_eval(layers, obs, actions=actions, mean=False, **pi)["logp"]
            ratio = torch.exp(new - old)
            clipped = ((ratio > 1 + CLIP) & (adv > 0)) | ((ratio < 1 - CLIP) & (adv < 0))
            c = torch.where(clipped, torch.zeros_like(adv), ratio * adv)
            state["clip_fraction"] = clipped.float().sum() / weights.sum()
            eng.policy_grad(layers, obs, actions, c, scale=1.0 / n, grad_out=grad, **pi)

        paths["fused"], paths["parts"] = fused, parts

    def policy_grad():
        eng.policy_grad(layers, obs, actions, adv, scale=1.0 / n, grad_out=grad, **pi)

    paths["policy_grad"] = policy_grad
    for fn in paths.values():
        for _ in range(2):
            timed(eng, fn)
    if not args.policy_grad_only:                    # the two ways agree (torch's exp is not the kernel's: to rounding, not bit for bit)
        fused()
        mine = grad.clone()
        parts()
        out["max_rel_difference"] = float((grad - mine).abs().max() / mine.abs().max())
        out["clip_fraction"] = float(state["res"]["clipped"] / state["res"]["used"])
        out["clip_fraction_parts"] = float(state["clip_fraction"])
    ms = {k: [] for k in paths}
    for _ in range(REPS):
        for k, fn in paths.items():
            ms[k].append(timed(eng, fn))
    out.update({k: stats(v) for k, v in ms.items()})
    if not args.policy_grad_only:
        a, b = out["fused"], out["parts"]
        out["parts_over_fused"] = round(b["median"] / a["median"], 3)
        out["separated"] = bool(abs(a["median"] - b["median"]) > max(a["spread"], b["spread"]))
        out["fused_ns_per_sample"] = round(a["median"] * 1e6 / (n * T), 4)
        out["fused_over_policy_grad"] = round(a["median"] / out["policy_grad"]["median"], 3)
    eng.close()
    torch.cuda.empty_cache()
    return out


def main():
    sizes = args.sizes or [65536, 1048576]
    res = {"T": T, "K": K, "table": "ref4", "reps": REPS, "clip": CLIP,
           "unit": "device ms per pass over the whole batch (T x N samples)"}
    parent = json.load(open(args.merge_parent)) if args.merge_parent else None
    for n in sizes:
        res[str(n)] = {}
        for n_layers, width in POLICIES:
            key = f"L{n_layers}" + (f"_w{width}" if n_layers > 1 else "")
            r = measure(n, n_layers, width)
            if parent is not None:
                p = parent[str(n)][key]["policy_grad"]
                r["parent_policy_grad"] = p
                r["policy_grad_over_parent"] = round(r["policy_grad"]["median"] / p["median"], 3)
                r["policy_grad_separated_from_parent"] = bool(abs(r["policy_grad"]["median"] - p["median"]) >
                                                              max(r["policy_grad"]["spread"], p["spread"]))
            res[str(n)][key] = r
            print(f"# n={n} {key}: {json.dumps(r)}", file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
