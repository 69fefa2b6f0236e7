#!/usr/bin/env python3
"""mt_ik and mt_jacobian against the parts a user writes without them: device time of ONE call -- 16 damped-least-squares
iterations at the defaults (damping 2, at most 30 degrees per iteration, no early stop, wrapped) -- at 65 536 / 1 048 576
arms of both built-in arms (the reference arm, the 7-joint arm; K = 7), with explicit targets and in nearest-target mode.

Per point, on ONE handle running on torch's stream, interleaved, REPS repeats after a warm-up, timed between two HIP events
on that stream (tools/es_sweep.py's protocol):
  ik        : one mt_ik through the C entry point, angles and residual written
  torch     : the same iteration restated with torch ops on (N, ...) tensors: batched sin / cos, one (N, 3, 3) bmm per joint
              for the chain, torch.linalg.cross per column, bmm for J J^T and J^T y, torch.linalg.solve on (N, 3, 3), the
              step cap, the wrap and the final residual; in nearest mode a masked argmin over the resident target rows first
  jacobian  : one mt_jacobian (Jacobian and driven point)
  jacobian_torch : the chain and the cross products of the torch restatement, stacked into (N, 3, D)
Both sides are checked against each other once per point (max |angles| difference of the settled envs is reported, not
asserted: tests/test_gpu_ik.py holds the kernel to fp64).  A pair counts as separated only if the medians differ by more
than the larger spread (max - min over the repeats).

    python tools/ik_sweep.py [--out profiles/ik_sweep.json] [sizes ...]"""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import manytor_amd as m  # noqa: E402

K, ITERS, REPS = 7, 16, 9
DAMPING, MAX_STEP = 2.0, 30.0
SEED = 0x1C5EED
ARMS = {"ref4": (m.REF_DH_TABLE, 51.3), "dh7": (m.DH7_TABLE, 51.3)}


def stats(us):
    s = sorted(us)
    return {"median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3), "spread": round(s[-1] - s[0], 3)}


class TorchArm:
    """The chain, the Jacobian and the DLS iteration of ik_kernel as torch ops over (N, ...) tensors."""

    def __init__(self, table, dev):
        self.rows = [tuple(float(v) for v in row) for row in table]
        self.dev = dev
        self.eye = torch.eye(3, device=dev)

    def chain(self, q):                                          # q (N, D) degrees
        n = q.shape[0]
        rot = self.eye.expand(n, 3, 3)
        pos = torch.zeros((n, 3), device=self.dev)
        zs, os_ = [], []
        for j, (a, alpha, d, off) in enumerate(self.rows):
            zs.append(rot[:, :, 2])
            os_.append(pos)
            th = torch.deg2rad(q[:, j]) + off
            ct, st = torch.cos(th), torch.sin(th)
            ca, sa = math.cos(alpha), math.sin(alpha)
            zero = torch.zeros_like(ct)
            mj = torch.stack([ct, -st * ca, st * sa, st, ct * ca, -ct * sa, zero, zero + sa, zero + ca], dim=1).view(n, 3, 3)
            local = torch.stack([a * ct, a * st, zero + d], dim=1)
            pos = pos + torch.bmm(rot, local.unsqueeze(2)).squeeze(2)
            rot = torch.bmm(rot, mj)
        return zs, os_, pos

    def jacobian(self, q):
        zs, os_, p = self.chain(q)
        return torch.stack([torch.linalg.cross(z, p - o) for z, o in zip(zs, os_)], dim=2), p      # (N, 3, D) per radian

    def ik(self, x, q):
        lam = DAMPING * DAMPING * self.eye
        for _ in range(ITERS):
            J, p = self.jacobian(q)
            e = (x - p).unsqueeze(2)
            y = torch.linalg.solve(torch.bmm(J, J.transpose(1, 2)) + lam, e)
            dq = torch.rad2deg(torch.bmm(J.transpose(1, 2), y).squeeze(2))
            mx = dq.abs().amax(dim=1, keepdim=True)
            q = q + dq * torch.where(mx > MAX_STEP, MAX_STEP / mx.clamp_min(1e-30), torch.ones_like(mx))
        q = q - 360.0 * torch.floor((q + 180.0) / 360.0)
        return q, (x - self.chain(q)[2]).abs().amax(dim=1)

    def nearest(self, points, alive, q):                         # points (3K, N) rows, alive (N,) bit mask
        p = self.chain(q)[2]
        pts = points.view(K, 3, -1).permute(2, 0, 1)             # (N, K, 3)
        d2 = ((pts - p.unsqueeze(1)) ** 2).sum(dim=2)
        live = (alive.unsqueeze(1) >> torch.arange(K, device=self.dev, dtype=alive.dtype)) & 1
        idx = torch.where(live.bool(), d2, torch.full_like(d2, float("inf"))).argmin(dim=1)
        return pts[torch.arange(pts.shape[0], device=self.dev), idx]


def draw_targets(n, radius, dev):
    rng = np.random.RandomState(SEED % 9973)
    out = np.empty((0, 3))
    while out.shape[0] < n:
        c = rng.uniform(-radius, radius, size=(2 * n + 16, 3))
        out = np.concatenate([out, c[(c[:, 2] >= 0) & (np.sqrt((c ** 2).sum(axis=1)) <= radius)]])
    return torch.from_numpy(np.ascontiguousarray(out[:n].T.astype(np.float32))).to(dev)          # (3, N)


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3          # us per call


def compare(out, ours, theirs):
    a, b = out[ours], out[theirs]
    out[f"{theirs}_over_{ours}"] = round(b["median"] / a["median"], 2)
    out[f"{theirs}_vs_{ours}_separated"] = bool(abs(a["median"] - b["median"]) > max(a["spread"], b["spread"]))


def measure(arm, n):
    table, radius = ARMS[arm]
    eng = m.StepEngine(n, K, dh_table=table, radius=radius)
    eng.use_torch_stream()
    eng.reset_random(SEED, 0)
    dev = torch.device("cuda", eng.device)
    d = eng.dof
    x = draw_targets(n, radius, dev)
    goals, points = eng.device_tensor(m.lib.F_GOALS), eng.device_tensor(m.lib.F_POINTS)
    alive = eng.device_tensor(m.lib.F_ALIVE)
    ang, res = torch.zeros((d, n), device=dev), torch.zeros(n, device=dev)
    jac, pos = torch.zeros((3 * d, n), device=dev), torch.zeros((3, n), device=dev)
    ta = TorchArm(table, dev)

    def ik_arg(target):
        s = m.lib.MtIk()
        s.struct_size, s.iters, s.damping, s.max_step_deg, s.tol = C.sizeof(m.lib.MtIk), ITERS, DAMPING, MAX_STEP, 0.0
        s.flags = m.lib.IK_WRAP
        s.target, s.target_ld = (target.data_ptr(), n) if target is not None else (None, 0)
        s.angles_out, s.angles_ld, s.residual_out = ang.data_ptr(), n, res.data_ptr()
        return s

    explicit, near = ik_arg(x), ik_arg(None)
    got = {}

    def torch_explicit():
        got["q"], got["r"] = ta.ik(x.t(), goals.t())

    def torch_nearest():
        got["q"], got["r"] = ta.ik(ta.nearest(points, alive, goals.t()), goals.t())

    paths = {
        "ik_explicit": lambda: m.lib.check(eng._lib.mt_ik(eng._h, C.byref(explicit)), eng._h),
        "torch_explicit": torch_explicit,
        "ik_nearest": lambda: m.lib.check(eng._lib.mt_ik(eng._h, C.byref(near)), eng._h),
        "torch_nearest": torch_nearest,
        "jacobian": lambda: m.lib.check(eng._lib.mt_jacobian(eng._h, None, 0, jac.data_ptr(), n, pos.data_ptr(), n), eng._h),
        "jacobian_torch": lambda: got.__setitem__("J", ta.jacobian(goals.t())),
    }
    for fn in paths.values():
        for _ in range(2):
            timed(fn, dev)
    us = {k: [] for k in paths}
    for _ in range(REPS):
        for k, fn in paths.items():
            us[k].append(timed(fn, dev))
    out = {k: stats(v) for k, v in us.items()}
    for mode in ("explicit", "nearest"):
        compare(out, f"ik_{mode}", f"torch_{mode}")
    compare(out, "jacobian", "jacobian_torch")
    # agreement of the two sides on the envs both put on the target (explicit targets)
    paths["ik_explicit"]()
    torch_explicit()
    torch.cuda.synchronize(dev)
    both = (res < 1e-3) & (got["r"] < 1e-3)
    diff = (ang.t() - got["q"])[both]
    diff = (diff - 360.0 * torch.round(diff / 360.0)).abs()
    out["on_target_share_kernel"] = round(float((res < 1e-3).float().mean()), 4)
    out["on_target_share_torch"] = round(float((got["r"] < 1e-3).float().mean()), 4)
    out["median_angle_difference_of_envs_on_target_deg"] = round(float(diff.amax(dim=1).median()), 5) if both.any() else None
    out["ik_explicit_us_per_iteration"] = round(out["ik_explicit"]["median"] / ITERS, 3)
    eng.close()
    del paths, got
    torch.cuda.empty_cache()
    return out


def main():
    argv = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "ik_sweep.json")
    if "--out" in argv:
        i = argv.index("--out")
        path = argv[i + 1]
        del argv[i:i + 2]
    sizes = [int(v) for v in argv] or [65536, 1048576]
    result = {"K": K, "iters": ITERS, "damping": DAMPING, "max_step": MAX_STEP, "reps": REPS, "unit": "device us per call"}
    for arm in ARMS:
        result[arm] = {}
        for n in sizes:
            result[arm][str(n)] = measure(arm, n)
            print(f"# {arm} n={n}: {json.dumps(result[arm][str(n)])}", file=sys.stderr, flush=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    main()
