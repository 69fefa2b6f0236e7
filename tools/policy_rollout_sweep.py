#!/usr/bin/env python3
"""mt_rollout_policy against the loop it replaces: device time per env-step of T = 20 steps of an MLP policy in the loop, at
65 536 / 1 048 576 arms of the reference arm (D = 4, K = 7), for policies of (L, width) = (1, -), (2, 32), (3, 32), (3, 64):
tanh hidden layers, a tanh output scaled to +-179 degrees, the same weights on every side.

Per point, on ONE handle running on torch's stream, interleaved, REPS repeats after a warm-up, timed between two HIP events
on that stream (tools/cem_sweep.py's protocol):
  fused        : one mt_rollout_policy of T steps through the C entry point, nothing logged
  parts        : T x (mt_observe; torch addmm + tanh per layer on the zero-copy views, the last into the staged actions;
                 mt_step) -- examples/policy_rollout.py --mode parts
  parts_graph  : the same round of launches captured once into a HIP graph, replayed T times
Every timed region starts from a freshly reset, idle handle.  A point counts as faster / slower only if the medians differ
by more than the larger spread (max - min over the repeats).

    python tools/policy_rollout_sweep.py [sizes ...] > profiles/policy_rollout_sweep.json"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import manytor_amd as m  # noqa: E402

T, K = 20, 7
POLICIES = ((1, 0), (2, 32), (3, 32), (3, 64))
REPS = 9
SEED = 0x7A9E
OUT_SCALE = 179.0


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


def fused_call(eng, layers):
    arg = m.lib.MtPolicy()
    arg.struct_size, arg.n_steps, arg.n_layers = C.sizeof(m.lib.MtPolicy), T, len(layers)
    for l, (w, b) in enumerate(layers):
        arg.weight[l], arg.bias[l] = w.data_ptr(), b.data_ptr()
        if l < len(layers) - 1:
            arg.width[l] = int(w.shape[0])
    arg.hidden_act = arg.out_act = m.lib.ACT_TANH
    arg.out_scale, arg.lo, arg.hi, arg.seed = OUT_SCALE, -180.0, 180.0, SEED

    def run():
        m.lib.check(eng._lib.mt_rollout_policy(eng._h, C.byref(arg)), eng._h)
    return run


def parts_round(eng, layers):
    obs, act = eng.device_tensor(m.lib.F_OBS), eng.device_tensor(m.lib.F_ACTIONS)

    def one():
        eng.observe()
        h = obs
        for w, b in layers[:-1]:
            h = torch.tanh(torch.addmm(b[:, None], w, h))
        w, b = layers[-1]
        torch.tanh(torch.addmm(b[:, None], w, h), out=act).mul_(OUT_SCALE)
        eng.step()
    return one


def parts_call(eng, layers):
    one = parts_round(eng, layers)

    def run():
        for _ in range(T):
            one()
    return run


def parts_graph_call(eng, layers):
    one = parts_round(eng, layers)
    for _ in range(3):
        one()
    torch.cuda.synchronize(eng.device)
    side = torch.cuda.Stream(device=eng.device)
    with torch.cuda.stream(side):
        eng.use_torch_stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            one()
    torch.cuda.synchronize(eng.device)
    eng.use_torch_stream()

    def run():
        for _ in range(T):
            g.replay()
    return run


def timed(eng, fn, episode):
    eng.reset_random(SEED, episode)
    torch.cuda.synchronize(eng.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / T          # us per step of the whole batch


def measure(n, n_layers, width):
    eng = m.StepEngine(n, K)
    eng.use_torch_stream()
    eng.reset_random(SEED, 0)
    layers = make_layers(eng, n_layers, width)
    paths = {"fused": fused_call(eng, layers), "parts": parts_call(eng, layers), "parts_graph": parts_graph_call(eng, layers)}
    for fn in paths.values():
        for _ in range(2):
            timed(eng, fn, 0)
    us = {k: [] for k in paths}
    for r in range(REPS):
        for k, fn in paths.items():
            us[k].append(timed(eng, fn, r + 1))
    out = {k: stats(v) for k, v in us.items()}
    for theirs in ("parts", "parts_graph"):
        a, b = out["fused"], out[theirs]
        out[f"{theirs}_over_fused"] = round(b["median"] / a["median"], 3)
        out[f"{theirs}_vs_fused_separated"] = bool(abs(a["median"] - b["median"]) > max(a["spread"], b["spread"]))
    out["fused_ns_per_env_step"] = round(out["fused"]["median"] * 1e3 / n, 4)
    sizes = [3 * K] + [width] * (n_layers - 1) + [eng.dof]
    out["fma_per_env_step"] = sum(i * o for i, o in zip(sizes[:-1], sizes[1:]))
    eng.close()
    del layers, paths
    torch.cuda.empty_cache()
    return out


def main():
    sizes = [int(v) for v in sys.argv[1:]] or [65536, 1048576]
    res = {"T": T, "K": K, "table": "ref4", "reps": REPS, "unit": "device us per step of the whole batch (call time / T)"}
    for n in sizes:
        res[str(n)] = {}
        for n_layers, width in POLICIES:
            key = f"L{n_layers}" + (f"_w{width}" if n_layers > 1 else "")
            res[str(n)][key] = measure(n, n_layers, width)
            print(f"# n={n} {key}: {json.dumps(res[str(n)][key])}", file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
