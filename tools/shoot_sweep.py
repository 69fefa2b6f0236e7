#!/usr/bin/env python3
"""mt_shoot against the calls it replaces: device time of ONE planning round -- score C candidate plans of T = 12 steps per
arm, pick each arm's best, commit its first H = 4 steps with auto-reset -- at 65 536 / 262 144 / 1 048 576 arms, C = 4, 8, 16,
for the reference arm (D = 4, K = 7) and the 7-joint table.

Per point, on ONE handle running on torch's stream, interleaved, REPS repeats after a warm-up, timed between two HIP events
on that stream:
  shoot    : one mt_shoot (evaluate + select, commit) through the C entry point, outputs allocated outside the region
  launches : what examples/plan_shooting.py --mode launches does per round -- C mt_rollout_tape dry runs into a (C, N) score
             tensor, torch argmax, the torch advanced-index gather of the chosen plans, the permute + copy into the tape
             layout, the committing mt_rollout_tape
Every timed region starts from a freshly reset, idle handle.  A point counts as faster / slower only if the medians differ
by more than the larger spread (max - min over the repeats).

    python tools/shoot_sweep.py [sizes ...] > profiles/shoot_sweep.json"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import manytor_amd as m  # noqa: E402

T, H, K = 12, 4, 7
CANDIDATES = (4, 8, 16)
REPS = 9
SEED = 0x7A9E


def stats(ms):
    s = sorted(ms)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4), "spread": round(s[-1] - s[0], 4)}


def make_plans(eng, c):
    dev = torch.device("cuda", eng.device)
    g = torch.Generator(device=dev)
    g.manual_seed(SEED)
    plans = torch.empty((c, T, eng.dof, eng.n_envs), device=dev)
    plans.uniform_(-180.0, 180.0, generator=g)
    plans[:, :, 1:3, :].mul_(0.4)                 # the example's shaping
    return plans


def shoot_call(eng, plans):
    n, c, dev = eng.n_envs, int(plans.shape[0]), plans.device
    best = torch.empty(n, dtype=torch.int32, device=dev)
    best_ret, ret = torch.empty(n, device=dev), torch.empty(n, device=dev)
    arg = m.lib.MtShoot()
    arg.struct_size, arg.n_steps, arg.n_candidates, arg.commit_steps = C.sizeof(m.lib.MtShoot), T, c, H
    arg.actions, arg.ld, arg.cand_stride = plans.data_ptr(), n, T * eng.dof * n
    arg.best_out, arg.best_return_out, arg.return_out = best.data_ptr(), best_ret.data_ptr(), ret.data_ptr()
    arg.seed, arg.flags = SEED, m.lib.SHOOT_AUTO_RESET

    def run(_keep=(best, best_ret, ret)):
        m.lib.check(eng._lib.mt_shoot(eng._h, C.byref(arg)), eng._h)
    return run


def launches_call(eng, plans):
    n, c, d, dev = eng.n_envs, int(plans.shape[0]), eng.dof, plans.device
    score = torch.empty((c, n), device=dev)
    ret = torch.empty(n, device=dev)
    envs = torch.arange(n, device=dev)
    dry = []
    for k in range(c):
        a = m.lib.MtTape()
        a.struct_size, a.n_steps, a.actions, a.ld = C.sizeof(m.lib.MtTape), T, plans[k].data_ptr(), n
        a.return_out, a.seed, a.flags = score[k].data_ptr(), SEED, m.lib.TAPE_DRY_RUN
        dry.append(a)
    real = m.lib.MtTape()
    real.struct_size, real.n_steps, real.ld = C.sizeof(m.lib.MtTape), H, n
    real.return_out, real.seed, real.flags = ret.data_ptr(), SEED, m.lib.TAPE_AUTO_RESET

    def run(_keep=(score, ret)):
        for a in dry:
            m.lib.check(eng._lib.mt_rollout_tape(eng._h, C.byref(a)), eng._h)
        best = score.argmax(dim=0)
        chosen = plans[best, :H, :, envs]                         # (N, H, D)
        tape = chosen.permute(1, 2, 0).contiguous()               # (H, D, N): what rollout_actions makes of it
        real.actions = tape.data_ptr()
        m.lib.check(eng._lib.mt_rollout_tape(eng._h, C.byref(real)), eng._h)
        return tape
    return run


def timed(eng, fn, episode):
    eng.reset_random(SEED, episode)
    torch.cuda.synchronize(eng.device)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    keep = fn()
    t1.record()
    t1.synchronize()
    del keep
    return t0.elapsed_time(t1)                    # ms per round


def measure(n, table, c):
    eng = m.StepEngine(n, K, dh_table=table, radius=51.3 if len(table) == 4 else 92.6, pickup_tol=20.0)
    eng.use_torch_stream()
    plans = make_plans(eng, c)
    paths = {"shoot": shoot_call(eng, plans), "launches": launches_call(eng, plans)}
    for fn in paths.values():
        for _ in range(2):
            timed(eng, fn, 0)
    ms = {k: [] for k in paths}
    for r in range(REPS):
        for k, fn in paths.items():
            ms[k].append(timed(eng, fn, r + 1))
    out = {k: stats(v) for k, v in ms.items()}
    a, b = out["shoot"], out["launches"]
    out["launches_over_shoot"] = round(b["median"] / a["median"], 3)
    out["separated"] = bool(abs(a["median"] - b["median"]) > max(a["spread"], b["spread"]))
    d = eng.dof
    # shoot: plans + the state once (pose, alive mask, targets) + best / best_return written + best and H rows read by the commit
    # launches: C x (plane + pose, alive mask, return, targets + the score row) + argmax (scores in, int64 out)
    #           + gather (index in, H rows in and out) + permute copy (in and out) + H rows read by the commit
    out["bytes_per_env"] = {"shoot": 4 * d * T * c + (4 * d + 4 + 12 * K) + 8 + 4 + 4 * d * H,
                            "launches": c * (4 * d * T + 4 * d + 8 + 12 * K + 4) + (4 * c + 8) + (8 + 8 * d * H) + 8 * d * H + 4 * d * H}
    eng.close()
    del plans
    torch.cuda.empty_cache()
    return out


def main():
    sizes = [int(v) for v in sys.argv[1:]] or [65536, 262144, 1048576]
    res = {"T": T, "H": H, "K": K, "reps": REPS, "unit": "device ms per planning round of the whole batch",
           "bytes_per_env_note": "evaluation and selection traffic of one round; the commit's own state traffic is the same on both sides and left out"}
    for name, table in (("ref4_k7", m.REF_DH_TABLE), ("dh7_k7", m.DH7_TABLE)):
        res[name] = {}
        for n in sizes:
            res[name][str(n)] = {}
            for c in CANDIDATES:
                res[name][str(n)][f"C{c}"] = measure(n, table, c)
                print(f"# {name} n={n} C={c}: {json.dumps(res[name][str(n)][f'C{c}'])}", file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
