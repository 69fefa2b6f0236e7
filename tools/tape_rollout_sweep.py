#!/usr/bin/env python3
"""mt_rollout_tape against the launch-per-step path it replaces: device us per env-step of T = 20 caller-chosen actions,
tape resident on the device, at 131 072 / 262 144 / 1 048 576 arms for the reference arm (D = 4, K = 7) and the
7-joint table.

Per size and table, on ONE handle, interleaved, REPS repeats after a warm-up (HIP events: mt_timer_start / mt_timer_stop):
  tape     : mt_rollout_tape with both logs and the returns (one launch)
  dry      : the same call as a dry run
  per_step : T x (mt_set_actions from a device (D, ld) row + mt_step), through the C entry points with no host wait in
             between -- what a caller had to do before mt_rollout_tape existed
and, on handles created with the overrides, the two optional choices of rollout_tape_kernel against the plain form:
  MT_TAPE_PREFETCH=1 (the tape row of step s + 1 requested before the kinematics of step s), MT_TAPE_NT=1 (non-temporal
  tape loads).  A choice is worth keeping only where the medians differ by more than the spread recorded beside them.

Every timed region starts from a freshly reset, idle handle (the reset is launched and waited for outside the region).

    python tools/tape_rollout_sweep.py [sizes ...] > profiles/r05_tape_rollout.json"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import manytor_amd as m  # noqa: E402

T = 20
REPS = 9
SEED = 0x7A9E


def stats(us):
    s = sorted(us)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4), "spread": round(s[-1] - s[0], 4)}


def engine(n, table, env=None):
    env = env or {}
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return m.StepEngine(n, 7, dh_table=table, radius=51.3 if len(table) == 4 else 92.6)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_tape(eng):
    import torch
    g = torch.Generator(device=f"cuda:{eng.device}")
    g.manual_seed(SEED)
    full = torch.rand((T, eng.dof, eng.ld), generator=g, device=f"cuda:{eng.device}", dtype=torch.float32) * 360.0 - 180.0
    torch.cuda.synchronize(eng.device)
    return full                                  # rows of pitch ld: each (D, ld) slice is what mt_set_actions(SOA) takes


def timed(eng, fn, episode):
    eng.reset_random(SEED, episode)
    eng.sync()                                   # (launches a deferred reset: outside the timed region)
    eng.timer_start()
    fn()
    return eng.timer_stop() * 1e3 / T            # us per step


def tape_call(eng, full, dry):
    """mt_rollout_tape through the C entry point, outputs allocated once outside the timed region (the Python front end
    allocates them per call and, on the handle's own stream, waits on the host around the launch)."""
    import torch
    n, dev = eng.n_envs, full.device
    keep = (torch.empty((T, n), dtype=torch.int8, device=dev), torch.empty((T, n), dtype=torch.uint8, device=dev),
            torch.empty(n, dtype=torch.float32, device=dev))
    torch.cuda.synchronize(dev)
    arg = m.lib.MtTape()
    arg.struct_size, arg.n_steps, arg.actions, arg.ld = C.sizeof(m.lib.MtTape), T, full.data_ptr(), eng.ld   # ld = the arena's row pitch
    arg.reward_log, arg.done_log, arg.log_ld, arg.return_out = keep[0].data_ptr(), keep[1].data_ptr(), n, keep[2].data_ptr()
    arg.seed, arg.flags = SEED, (m.lib.TAPE_DRY_RUN if dry else 0)

    def run(_keep=keep):
        m.lib.check(eng._lib.mt_rollout_tape(eng._h, C.byref(arg)), eng._h)
    return run


def per_step_call(eng, full):
    lib, h = eng._lib, eng._h
    rows = [C.c_void_p(full[t].data_ptr()) for t in range(T)]

    def run():
        for t in range(T):
            m.lib.check(lib.mt_set_actions(h, rows[t], m.lib.DT_F32, m.lib.SOA, 1), h)
            m.lib.check(lib.mt_step(h), h)
    return run


def measure(n, table):
    eng = engine(n, table)
    full = make_tape(eng)
    paths = {"tape": tape_call(eng, full, False), "dry": tape_call(eng, full, True), "per_step": per_step_call(eng, full)}
    for fn in paths.values():                    # warm-up: every path twice
        for _ in range(2):
            timed(eng, fn, 0)
    us = {k: [] for k in paths}
    for r in range(REPS):
        for k, fn in paths.items():
            us[k].append(timed(eng, fn, r + 1))
    out = {k: stats(v) for k, v in us.items()}
    out["dispatch"] = {"step": eng.step_kernel_name(), "chains": eng.dispatch()["chains"]["count"]}
    out["tape_vs_per_step"] = round(out["per_step"]["median"] / out["tape"]["median"], 3)
    eng.close()

    # the two optional kernel choices, each on a handle of its own, interleaved with the plain form
    variants = {"plain": {}, "prefetch": {"MT_TAPE_PREFETCH": "1"}, "nt": {"MT_TAPE_NT": "1"},
                "prefetch_nt": {"MT_TAPE_PREFETCH": "1", "MT_TAPE_NT": "1"}}
    engs = {k: engine(n, table, env) for k, env in variants.items()}
    calls = {k: tape_call(e, full, False) for k, e in engs.items()}
    for k, e in engs.items():
        for _ in range(2):
            timed(e, calls[k], 0)
    vus = {k: [] for k in variants}
    for r in range(REPS):
        for k, e in engs.items():
            vus[k].append(timed(e, calls[k], r + 1))
    out["choices"] = {k: stats(v) for k, v in vus.items()}
    for k in ("prefetch", "nt", "prefetch_nt"):
        a, b = out["choices"]["plain"], out["choices"][k]
        out["choices"][k]["gain_us"] = round(a["median"] - b["median"], 4)
        out["choices"][k]["separated"] = bool(abs(a["median"] - b["median"]) > max(a["spread"], b["spread"]))
    for e in engs.values():
        e.close()
    return out


def main():
    sizes = [int(v) for v in sys.argv[1:]] or [131072, 262144, 1048576]
    res = {"T": T, "reps": REPS, "unit": "device us per step of the whole batch", "byte_model_per_env_step":
           {"tape_d4": 4 * 4 + 2, "tape_d7": 4 * 7 + 2, "mt_step_d4_k7": 249}}
    for name, table in (("ref4_k7", m.REF_DH_TABLE), ("dh7_k7", m.DH7_TABLE)):
        res[name] = {}
        for n in sizes:
            res[name][str(n)] = measure(n, table)
            print(f"# {name} n={n}: {json.dumps(res[name][str(n)])}", file=sys.stderr, flush=True)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
