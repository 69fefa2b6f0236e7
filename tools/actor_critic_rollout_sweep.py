#!/usr/bin/env python3
"""mt_rollout_actor_critic against the five calls it replaces in an actor-critic collection, and mt_rollout_policy alone
(whose instantiations the new mode must not have slowed down): device time of T = 20 steps at 65 536 / 1 048 576 arms of
the reference arm (D = 4, K = 7), policy and critic alike of (L, width) = (1, -), (2, 32), (3, 32), (3, 64), the points of
tools/ppo_grad_sweep.py.

Per point, on ONE handle running on torch's stream, interleaved, REPS repeats after a warm-up of every path, timed between
two HIP events on that stream around a synchronised region (tools/ppo_grad_sweep.py's protocol):
  fused    one rollout_policy(logp=True, critic=, log, actions, observations): mt_rollout_actor_critic, one launch
  parts    rollout_policy with the same logs; policy_eval(mean=False) for log pi_old; values(obs); observe() and values on the
           resident observation rows for V(x_T): five launches, the observation log read twice more
  rollout  mt_rollout_policy alone with the same logs (the same call on this commit and on the parent)
Every path starts from the same state (dry_run=True: nothing resident changes, the work is the same).  A point counts as
faster / slower only if the medians differ by more than the larger spread (max - min over the repeats).

    python tools/actor_critic_rollout_sweep.py [sizes ...] > profiles/actor_critic_rollout_sweep.json
    python tools/actor_critic_rollout_sweep.py --rollout-only --root PARENT_CHECKOUT [sizes ...]    # the parent's mt_rollout_policy

With --merge-parent FILE the output of the second command is attached to the first as `parent_rollout` per point."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("sizes", nargs="*", type=int)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the built tree whose manytor_amd is measured (default: this one)")
ap.add_argument("--rollout-only", action="store_true", help="time mt_rollout_policy alone (all a parent checkout has)")
ap.add_argument("--merge-parent", default=None, help="a --rollout-only result of the parent commit to record beside this one")
args = ap.parse_args()

import torch  # noqa: E402

sys.path.insert(0, args.root)
import manytor_amd as m  # noqa: E402

T, K = 20, 7
NETS = ((1, 0), (2, 32), (3, 32), (3, 64))
REPS = 9
SEED = 0x7A9E
OUT_SCALE = 179.0
SIGMA = 15.0


def stats(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4), "spread": round(s[-1] - s[0], 4)}


def make_layers(eng, n_layers, width, n_out, seed):
    dev = torch.device("cuda", eng.device)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    n_in = 3 * K
    sizes = [n_in] + [width] * (n_layers - 1) + [n_out]
    return [(torch.randn(o, i, device=dev, generator=g) * (1.0 / (60.0 * n_in ** 0.5) if l == 0 else i ** -0.5),
             torch.randn(o, device=dev, generator=g) * 0.1) for l, (i, o) in enumerate(zip(sizes[:-1], sizes[1:]))]


def timed(eng, fn):
    torch.cuda.synchronize(eng.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)          # ms per collection of the whole batch


def measure(n, n_layers, width):
    eng = m.StepEngine(n, K)
    eng.use_torch_stream()
    eng.reset_random(SEED, 0)
    layers = make_layers(eng, n_layers, width, eng.dof, SEED)
    critic = make_layers(eng, n_layers, width, 1, SEED + 1)
    kw = dict(sigma=SIGMA, seed=SEED, out_scale=OUT_SCALE, log=True, actions=True, observations=True, dry_run=True)
    paths, out, state = {}, {}, {}
    if not args.rollout_only:
        def fused():
            state["fused"] = eng.rollout_policy(layers, T, logp=True, critic=critic, **kw)

        def parts():
            log = eng.rollout_policy(layers, T, **kw)
            obs = log["observations"]
            logp = eng.policy_eval(layers, obs, actions=log["actions"], sigma=SIGMA, out_scale=OUT_SCALE, mean=False)["logp"]
            values = eng.values(critic, obs)
            eng.observe()
            last = eng.values(critic, eng.device_tensor(m.lib.F_OBS)[None])[0]
            state["parts"] = dict(logp=logp, values=values, last_value=last)

        paths["fused"], paths["parts"] = fused, parts

    def rollout():
        eng.rollout_policy(layers, T, **kw)

    paths["rollout"] = rollout
    for fn in paths.values():
        for _ in range(2):
            timed(eng, fn)
    if not args.rollout_only:                        # the two ways agree bit for bit (x_T of a dry run is the state it started from)
        out["bit_equal"] = bool(all(torch.equal(state["fused"][k], state["parts"][k]) for k in ("logp", "values")))
    ms = {k: [] for k in paths}
    for _ in range(REPS):
        for k, fn in paths.items():
            ms[k].append(timed(eng, fn))
    out.update({k: stats(v) for k, v in ms.items()})
    if not args.rollout_only:
        a, b = out["fused"], out["parts"]
        out["parts_over_fused"] = round(b["median"] / a["median"], 3)
        out["separated"] = bool(abs(a["median"] - b["median"]) > max(a["spread"], b["spread"]))
        out["fused_over_rollout"] = round(a["median"] / out["rollout"]["median"], 3)
    eng.close()
    torch.cuda.empty_cache()
    return out


def main():
    sizes = args.sizes or [65536, 1048576]
    res = {"T": T, "K": K, "table": "ref4", "reps": REPS,
           "unit": "device ms per collection of the whole batch (T steps x N arms), every log written"}
    parent = json.load(open(args.merge_parent)) if args.merge_parent else None
    for n in sizes:
        res[str(n)] = {}
        for n_layers, width in NETS:
            key = f"L{n_layers}" + (f"_w{width}" if n_layers > 1 else "")
            r = measure(n, n_layers, width)
            if parent is not None:
                p = parent[str(n)][key]["rollout"]
                r["parent_rollout"] = p
                r["rollout_over_parent"] = round(r["rollout"]["median"] / p["median"], 3)
                r["rollout_separated_from_parent"] = bool(abs(r["rollout"]["median"] - p["median"]) >
                                                          max(r["rollout"]["spread"], p["spread"]))
            res[str(n)][key] = r
            print(f"# n={n} {key}: {json.dumps(r)}", file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
