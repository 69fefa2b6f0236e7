"""StepEngine: thin object wrapper over one mt_handle (include/manytor_hip.h).

One engine = N lock-stepped arms resident on one MI355X.  All arithmetic runs in
the HIP kernels; this file only marshals arguments.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib as L

# DH rows (a, alpha, d, theta_offset) of the reference arm, manytor.py:42-48.
REF_DH_TABLE = (
    (0.0, -math.pi / 2, 4.3, 0.0),
    (0.0, math.pi / 2, 0.0, 0.0),
    (0.0, -math.pi / 2, 24.3, 0.0),
    (27.0, math.pi / 2, 0.0, -math.pi / 2),
)

# A 7-joint table for the generalised-DH configuration (BASELINE.json configs[4]);
# pinned by fixture F7 (tests/golden/f7_dh7_kat.npz).
DH7_TABLE = (
    (0.0, -math.pi / 2, 34.0, 0.0),
    (0.0, math.pi / 2, 0.0, 0.0),
    (4.5, math.pi / 2, 40.0, 0.0),
    (-4.5, -math.pi / 2, 0.0, 0.0),
    (0.0, -math.pi / 2, 40.0, 0.0),
    (8.8, math.pi / 2, 0.0, -math.pi / 2),
    (0.0, 0.0, 12.6, 0.0),
)

_NP_OF_DT = {L.DT_F32: np.float32, L.DT_I32: np.int32, L.DT_U8: np.uint8, L.DT_U32: np.uint32, L.DT_U64: np.uint64}
_TYPESTR = {L.DT_F32: "<f4", L.DT_I32: "<i4", L.DT_U8: "|u1", L.DT_U32: "<u4", L.DT_U64: "<u8"}
_ACTION_DT = {np.dtype(np.float32): L.DT_F32, np.dtype(np.float64): L.DT_F64, np.dtype(np.int32): L.DT_I32,
              np.dtype(np.int64): L.DT_I64}


def _is_torch_tensor(x) -> bool:
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


class _CudaArrayHolder:
    """Exposes a raw device range through __cuda_array_interface__ (consumed by torch.as_tensor)."""

    def __init__(self, ptr, shape, strides, typestr, owner):
        self.__cuda_array_interface__ = {
            "shape": tuple(shape), "strides": tuple(strides), "typestr": typestr, "data": (int(ptr), False), "version": 2,
        }
        self._owner = owner     # keeps the engine (and its arena) alive


class StepEngine:
    """N lock-stepped manipulator envs on one GPU.

    Mirrors, for a batch, the state and methods of the reference ``Environment``
    (manytor.py:125-260): reset / step / get_observations / is_done /
    action_sample.  Field getters return arrays in the reference's shapes with a
    leading env axis.
    """

    def __init__(self, n_envs, obj_number=10, dh_table=REF_DH_TABLE, substeps=25, pickup_tol=8.0, radius=51.3,
                 device=0, env_id_base=0, terminate_on_ground=False, hw_trig=False, dh_in_lds=False,
                 direct_trig=False, specialize=True, ablate=0, return_ring=4, trace=False, obs_frame=-2, ee_frame=-1,
                 debug_zmin=False):
        self._lib = L.load()
        table = np.asarray(dh_table, dtype=np.float64)
        if table.ndim != 2 or table.shape[1] != 4:
            raise ValueError("dh_table must be (dof, 4): rows (a, alpha, d, theta_offset)")
        self.n_envs = int(n_envs)
        self.obj_number = int(obj_number)
        self.dof = int(table.shape[0])
        self.substeps = int(substeps)
        self.device = int(device)
        self.env_id_base = int(env_id_base)
        self.dh_table = table
        cfg = L.MtConfig()
        cfg.struct_size = C.sizeof(L.MtConfig)
        cfg.device = self.device
        cfg.n_envs = self.n_envs
        cfg.env_id_base = self.env_id_base
        cfg.dof = self.dof
        cfg.n_targets = self.obj_number
        cfg.substeps = self.substeps
        cfg.flags = ((L.FLAG_TERMINATE_ON_GROUND if terminate_on_ground else 0) | (L.FLAG_HW_TRIG if hw_trig else 0)
                     | (L.FLAG_DH_IN_LDS if dh_in_lds else 0) | (L.FLAG_DIRECT_TRIG if direct_trig else 0)
                     | (0 if specialize else L.FLAG_NO_SPECIALIZE) | (L.FLAG_TRACE if trace else 0)
                     | (L.FLAG_DEBUG_ZMIN if debug_zmin else 0)
                     | (L.FLAG_ABLATE_LOOP if ablate in (1, 2) else 0) | (L.FLAG_ABLATE_OBS if ablate in (2, 3) else 0))
        cfg.pickup_tol = float(pickup_tol)
        cfg.radius = float(radius)
        cfg.return_ring = int(return_ring)
        cfg.obs_frame = int(obs_frame)      # rows of joints_coordinates: observation from [-2], pickup from [-1] in the
        cfg.ee_frame = int(ee_frame)        # reference (manytor.py:143, :162); selectable for other arms
        cfg.reserved = 0
        self.return_ring_slots = int(return_ring)
        self.has_trace = bool(trace)
        self.episode0 = 0         # episode index every env got at the last full reset
        if self.dof > L.MT_MAX_DOF:
            raise ValueError(f"dof must be <= {L.MT_MAX_DOF}")
        flat = table.astype(np.float32).ravel()
        for i, v in enumerate(flat):
            cfg.dh_table[i] = float(v)
        self._h = L._HANDLE()
        L.check(self._lib.mt_create(C.byref(self._h), C.byref(cfg)))
        self.version = 0          # bumped by every call that changes device state (host caches key on it)

    # ---- lifetime ---------------------------------------------------------------------------
    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.mt_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _call(self, fn, *args):
        if not self._h:
            raise RuntimeError("StepEngine is closed")
        L.check(fn(self._h, *args), self._h)

    def step_kernel_name(self) -> str:
        """The kernel instantiation step() / step_random() launch for this batch (schedule picked at construction)."""
        if not self._h:
            raise RuntimeError("StepEngine is closed")
        return self._lib.mt_step_kernel_name(self._h).decode()

    def dispatch(self) -> dict:
        """The dispatch of this engine as data (mt_describe_dispatch): the schedule resolved for every entry point, the
        MT_* overrides in effect and the library's table of size thresholds."""
        import json
        if not self._h:
            raise RuntimeError("StepEngine is closed")
        return json.loads(self._lib.mt_describe_dispatch(self._h).decode())

    # ---- stream / sync / timing ---------------------------------------------------------------
    def set_stream(self, hip_stream):
        """Run on a caller-owned hipStream_t (int / pointer).  0 is the legacy default stream (torch's default
        stream); None goes back to the engine's own private stream, which is ordered against nothing else."""
        if hip_stream is None:
            self._call(self._lib.mt_use_own_stream)
        else:
            self._call(self._lib.mt_set_stream, C.c_void_p(int(hip_stream)))
        self._caller_stream = None if hip_stream is None else int(hip_stream)

    def use_torch_stream(self):
        """Launch on torch's current stream of this device: torch ops on that stream (device_tensor views, RCCL
        collectives) and engine launches then execute in program order, no manual sync needed."""
        import torch
        self.set_stream(int(torch.cuda.current_stream(self.device).cuda_stream))

    def sync(self):
        self._call(self._lib.mt_sync)

    def timer_start(self):
        self._call(self._lib.mt_timer_start)

    def timer_stop(self) -> float:
        ms = C.c_float(0)
        self._call(self._lib.mt_timer_stop, C.byref(ms))
        return ms.value

    def timer_stop_async(self):
        """End mark of timer_start without joining the chains or waiting on the host; timer_read() waits and returns."""
        self._call(self._lib.mt_timer_stop_async)

    def timer_read(self) -> float:
        """Device milliseconds from timer_start to the last end event of timer_stop_async (all streams of the engine,
        incl. an exchange that was pending on the side stream)."""
        ms = C.c_float(0)
        self._call(self._lib.mt_timer_read, C.byref(ms))
        return ms.value

    def lap_begin(self):
        self._call(self._lib.mt_timer_lap_begin)

    def lap_end(self):
        self._call(self._lib.mt_timer_lap_end)

    def laps_total(self):
        """(summed device milliseconds of all laps since the last call, number of laps); synchronises once."""
        ms, n = C.c_float(0), C.c_int(0)
        self._call(self._lib.mt_timer_laps_total, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def lap_times(self):
        """Device milliseconds of every lap since the last call, in recording order; synchronises once."""
        cap = 4096
        while True:
            buf, n = (C.c_float * cap)(), C.c_int(0)
            rc = self._lib.mt_timer_lap_times(self._h, buf, cap, C.byref(n))
            if rc != L.MT_OK and n.value > cap:
                cap = n.value
                continue
            L.check(rc, self._h)
            return list(buf[: n.value])

    # ---- reset --------------------------------------------------------------------------------
    def reset(self, points):
        """Environment.reset (manytor.py:219-253) with caller-supplied targets: (N, K, 3) host array
        or device tensor (env-major), or a (3K, ld) float32 device tensor (SoA)."""
        n, k = self.n_envs, self.obj_number
        if _is_torch_tensor(points):
            import torch
            t = points
            if not t.is_cuda:
                return self.reset(t.detach().cpu().numpy())
            if t.dtype != torch.float32 or not t.is_contiguous():
                t = t.to(torch.float32).contiguous()
            if t.numel() == n * k * 3:
                layout = L.ENV_MAJOR
            elif tuple(t.shape) == (3 * k, self.ld):
                layout = L.SOA
            else:
                raise ValueError("device points must be (N,K,3) or (3K, ld)")
            torch.cuda.current_stream(self.device).synchronize()
            self._call(self._lib.mt_reset, C.c_void_p(t.data_ptr()), layout, 1)
            self.sync()
        else:
            p = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(n, k, 3))
            self._call(self._lib.mt_reset, p.ctypes.data_as(C.c_void_p), L.ENV_MAJOR, 0)
        self.episode0 = 0
        self._armed = True
        self.version += 1

    def reset_random(self, seed=0x5EED, episode=0):
        self._call(self._lib.mt_reset_random, C.c_uint64(seed), C.c_uint32(episode))
        self.episode0 = int(episode)
        self._armed = True
        self.version += 1

    def env_reset(self, env, points=None, seed=0x5EED, episode=0):
        """``multienv.environment[env].reset()`` (manytor.py:82 + :219-253): reset ONE env; `points` (K, 3) or None
        to draw them on the device."""
        p = None
        if points is not None:
            p = np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(self.obj_number, 3))
        self._call(self._lib.mt_env_reset, C.c_int64(int(env)), p.ctypes.data_as(C.c_void_p) if p is not None else None,
                   C.c_uint64(seed), C.c_uint32(episode))
        self.version += 1

    def reset_done(self, seed=0x5EED):
        """Re-arm the envs whose done flag is set (new targets keyed by their own episode counter)."""
        self._call(self._lib.mt_reset_done, C.c_uint64(seed))
        self.version += 1

    # ---- actions ------------------------------------------------------------------------------
    def set_actions(self, actions):
        """(N, D) degrees: nested lists, numpy (f32/f64/i32/i64) or a device tensor; or (D, ld) SoA device tensor."""
        n, d = self.n_envs, self.dof
        if _is_torch_tensor(actions) and actions.is_cuda:
            import torch
            t = actions
            dt = {torch.float32: L.DT_F32, torch.float64: L.DT_F64, torch.int32: L.DT_I32, torch.int64: L.DT_I64}.get(t.dtype)
            if dt is None:
                t, dt = t.to(torch.float32), L.DT_F32
            t = t.contiguous()
            if tuple(t.shape) == (n, d):
                layout = L.ENV_MAJOR
            elif tuple(t.shape) == (d, self.ld):
                layout = L.SOA
            else:
                raise ValueError(f"device actions must be ({n},{d}) or ({d},{self.ld})")
            torch.cuda.current_stream(self.device).synchronize()
            self._call(self._lib.mt_set_actions, C.c_void_p(t.data_ptr()), dt, layout, 1)
            self.sync()
            return
        if _is_torch_tensor(actions):
            actions = actions.detach().cpu().numpy()
        a = np.asarray(actions)
        if a.dtype not in _ACTION_DT:
            a = a.astype(np.float64)
        if a.size != n * d:
            raise ValueError(f"actions must have {n}x{d} elements, got shape {a.shape}")
        a = np.ascontiguousarray(a.reshape(n, d))
        self._call(self._lib.mt_set_actions, a.ctypes.data_as(C.c_void_p), _ACTION_DT[a.dtype], L.ENV_MAJOR, 0)

    def sample_actions(self, seed=0x5EED, step_idx=0):
        """Environment.action_sample (manytor.py:215-217) on the device, into the action buffer."""
        self._call(self._lib.mt_sample_actions, C.c_uint64(seed), C.c_uint32(step_idx))

    # ---- step ---------------------------------------------------------------------------------
    def step(self, actions=None):
        """Environment.step (manytor.py:255-260) for all envs.  Results stay on the device:
        read them with get()/device_tensor()."""
        if actions is not None:
            self.set_actions(actions)
        self._call(self._lib.mt_step)
        self.version += 1

    def step_host(self, actions):
        """One host round trip: (N, D) host actions in -> (obs2 (N, 3K) f32, reward (N,) i32, done (N,) bool) out,
        with a single synchronisation.  The small-batch path of the drop-in classes."""
        n, d = self.n_envs, self.dof
        a = np.asarray(actions)
        if a.dtype not in _ACTION_DT:
            a = a.astype(np.float64)
        if a.size != n * d:
            raise ValueError(f"actions must have {n}x{d} elements, got shape {a.shape}")
        a = np.ascontiguousarray(a.reshape(n, d))
        obs = np.empty((n, 3 * self.obj_number), dtype=np.float32)
        rew = np.empty(n, dtype=np.int32)
        done = np.empty(n, dtype=np.uint8)
        self._call(self._lib.mt_step_host, a.ctypes.data_as(C.c_void_p), _ACTION_DT[a.dtype],
                   obs.ctypes.data_as(C.c_void_p), rew.ctypes.data_as(C.c_void_p), done.ctypes.data_as(C.c_void_p))
        self.version += 1
        return obs, rew, done.astype(bool)

    def env_step(self, env, action):
        """``multienv.environment[env].step(action)`` (manytor.py:82,118): step ONE env of the batch, the others are
        untouched -> (obs2 (3K,) f32, reward int, done bool)."""
        a = np.ascontiguousarray(np.asarray(action, dtype=np.float32).reshape(self.dof))
        obs = np.empty(3 * self.obj_number, dtype=np.float32)
        rew, done = C.c_int32(0), C.c_uint8(0)
        self._call(self._lib.mt_env_step, C.c_int64(int(env)), a.ctypes.data_as(C.c_void_p), obs.ctypes.data_as(C.c_void_p),
                   C.byref(rew), C.byref(done))
        self.version += 1
        return obs, int(rew.value), bool(done.value)

    def bad_action_count(self) -> int:
        """How many (env, step) pairs so far were handed a non-finite / absurd action and held their pose instead."""
        c = C.c_uint64(0)
        self._call(self._lib.mt_bad_action_count, C.byref(c))
        return int(c.value)

    def step_random(self, seed=0x5EED, step_idx=0):
        self._call(self._lib.mt_step_random, C.c_uint64(seed), C.c_uint32(step_idx))
        self.version += 1

    def rollout(self, n_steps, seed=0x5EED, step_idx0=0):
        self._call(self._lib.mt_rollout, int(n_steps), C.c_uint64(seed), C.c_uint32(step_idx0))
        self.version += 1

    def rollout_fused(self, n_steps, seed=0x5EED, step_idx0=0, auto_reset=False):
        """n_steps random-action steps in ONE launch (state in registers / LDS between steps)."""
        self._call(self._lib.mt_rollout_fused, int(n_steps), C.c_uint64(seed), C.c_uint32(step_idx0),
                   1 if auto_reset else 0)
        self.version += 1

    def _tape_tensor(self, actions, layout, candidates=False):
        """(tensor, ld) of a device action tape in the kernel's layout: f32, joint j of env i at step t at
        [(t * D + j) * ld + i].  A CUDA f32 (T, D, N) tensor with unit env stride and a uniform row pitch >= N goes in
        zero-copy; anything else becomes a contiguous (T, D, N) f32 tensor on the engine's device.
        candidates=True: a stack of C such tapes, (C, T, D, N) or (C, T, N, D) -> (tensor, ld, cand_stride); read in place
        under the same conditions when the candidate stride is uniform and the planes do not overlap."""
        import torch
        n, d = self.n_envs, self.dof
        lead = "C, T" if candidates else "T"
        if layout not in ("env_major", "soa"):
            raise ValueError(f"layout must be 'env_major' ({lead}, N, D) or 'soa' ({lead}, D, N)")
        dev = torch.device("cuda", self.device)
        if _is_torch_tensor(actions):
            t = actions.detach()
        else:
            a = np.asarray(actions)
            if a.dtype not in _ACTION_DT:
                a = a.astype(np.float64)
            a = np.ascontiguousarray(a)
            t = torch.from_numpy(a if a.flags.writeable else a.copy())
        nd = 4 if candidates else 3
        if t.dim() != nd or tuple(t.shape[-2:]) != ((d, n) if layout == "soa" else (n, d)):
            want = f"({lead}, {d}, {n})" if layout == "soa" else f"({lead}, {n}, {d})"
            what = "plans" if candidates else "actions"
            raise ValueError(f"{what} must be {want} for layout={layout!r}, got {tuple(t.shape)}")
        if not candidates:
            if t.shape[0] == 0:
                return torch.empty((0, d, n), dtype=torch.float32, device=dev), n
            if (layout == "soa" and t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.stride(2) == 1
                    and t.stride(1) >= n and t.stride(0) == d * t.stride(1)):
                return t, int(t.stride(1))
            t = t.to(device=dev, dtype=torch.float32)
            if layout == "env_major":
                t = t.permute(0, 2, 1)
            return t.contiguous(), n
        c, steps = int(t.shape[0]), int(t.shape[1])
        if c == 0 or steps == 0:
            return torch.empty((c, steps, d, n), dtype=torch.float32, device=dev), n, steps * d * n
        if (layout == "soa" and t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.stride(3) == 1
                and t.stride(2) >= n and t.stride(1) == d * t.stride(2) and t.stride(0) >= steps * t.stride(1)):
            return t, int(t.stride(2)), int(t.stride(0))
        t = t.to(device=dev, dtype=torch.float32)
        if layout == "env_major":
            t = t.permute(0, 1, 3, 2)
        return t.contiguous(), n, steps * d * n

    def _torch_call(self, fn, *args, commits):
        """A library call that reads and writes torch's memory: on torch's stream (use_torch_stream) it is ordered with the
        torch ops around it and waits for nothing; on the engine's own stream it waits for torch's current stream before
        and for its own launch after.  commits: the call changes the resident state."""
        import torch
        cur = torch.cuda.current_stream(self.device)
        ordered = getattr(self, "_caller_stream", None) == int(cur.cuda_stream)   # the engine launches on torch's current stream
        if not ordered:
            cur.synchronize()
        self._call(fn, *args)
        if not ordered:
            self.sync()     # the inputs and the outputs are torch's memory: done with before torch may reuse or read it
        if commits:
            self.version += 1

    @staticmethod
    def _commit_steps(commit, auto_reset):
        """A planner's `commit` as an int; refused ahead of everything else when auto_reset has nothing to re-arm."""
        commit = int(commit)
        if auto_reset and commit == 0:
            raise ValueError("auto_reset needs commit > 0: an evaluation re-arms nothing")
        return commit

    def _commit_outputs(self, arg, out, T, commit, log, returns, chosen=True):
        """The commit side of shoot / cem / mppi: `commit` against T, then the outputs of the committed steps into `out` and
        their addresses into `arg` (`chosen`: the call writes the committed angles as a tape of their own)."""
        import torch
        if not 0 <= commit <= T:
            raise ValueError(f"commit must be 0..T = {T}, got {commit}")
        n, dev = self.n_envs, out["best"].device
        arg.commit_steps = commit
        if chosen:
            if commit:
                out["chosen"] = torch.empty((commit, self.dof, n), dtype=torch.float32, device=dev)
            arg.chosen_out = out["chosen"].data_ptr() if commit else None
            arg.chosen_ld = n
        if log:
            out["reward"] = torch.empty((commit, n), dtype=torch.int8, device=dev)
            out["done"] = torch.empty((commit, n), dtype=torch.uint8, device=dev)
        if returns:                                              # (commit == 0: the call writes nothing here)
            out["returns"] = (torch.empty if commit else torch.zeros)(n, dtype=torch.float32, device=dev)
        arg.reward_log = out["reward"].data_ptr() if log and commit else None
        arg.done_log = out["done"].data_ptr() if log and commit else None
        arg.log_ld = n
        arg.return_out = out["returns"].data_ptr() if returns and commit else None

    def _refit_args(self, arg, mean, sigma, c, lo, hi, sigma_min, draw, seed, inplace, fit_sigma, all_returns, max_steps=None):
        """What cem and mppi share ahead of the commit: sigma_min, the horizon (max_steps: the call's own limit, ahead of the
        tensor checks) and the rows; the candidate stream and the refit's outputs into `arg`.  Returns (out, T, alloc),
        alloc(shape, dtype=) for the further outputs the kernel writes whenever it runs."""
        import functools
        import torch
        sigma_min = float(sigma_min)
        if not (np.isfinite(sigma_min) and sigma_min >= 0.0):
            raise ValueError(f"sigma_min must be finite and >= 0, got {sigma_min}")
        steps = getattr(mean, "shape", None)
        if max_steps is not None and steps is not None and len(steps) == 3 and int(steps[0]) > max_steps:
            raise ValueError(f"at most {max_steps} steps, got {int(steps[0])}")
        mean, sigma, T, ld = self._cem_rows(mean, sigma)
        n, d = self.n_envs, self.dof
        dev = mean.device
        alloc = functools.partial(torch.empty if T else torch.zeros, device=dev)   # (T == 0: the call is a no-op and writes nothing)
        out = {"best": alloc(n, dtype=torch.int32), "best_return": alloc(n, dtype=torch.float32)}
        fitted = ("mean", "sigma") if fit_sigma else ("mean",)
        for name, t in zip(fitted, (mean, sigma)):
            out[name] = t if inplace else torch.empty((T, d, n), dtype=torch.float32, device=dev)
        if all_returns:
            out["candidate_returns"] = alloc((c, n), dtype=torch.float32)
        arg.n_steps, arg.n_candidates, arg.draw = T, c, int(draw) & 0xFFFFFFFF
        arg.mean, arg.sigma, arg.ld = (mean.data_ptr(), sigma.data_ptr(), ld) if T else (None, None, n)
        arg.mean_out = out["mean"].data_ptr() if T else None
        arg.sigma_out = out["sigma"].data_ptr() if T and fit_sigma else None
        arg.out_ld = ld if inplace else n
        arg.lo, arg.hi, arg.sigma_min = lo, hi, sigma_min
        arg.returns_out = out["candidate_returns"].data_ptr() if all_returns else None
        arg.ret_ld = n
        arg.best_out = out["best"].data_ptr()
        arg.best_return_out = out["best_return"].data_ptr()
        arg.seed = int(seed)
        return out, T, alloc

    def rollout_actions(self, actions, *, layout="env_major", auto_reset=False, seed=0x5EED, log=False, returns=False,
                        dry_run=False):
        """T steps with the caller's actions in ONE launch (mt_rollout_tape): `actions` is (T, N, D) degrees
        (layout="env_major") or (T, D, N) (layout="soa"; a CUDA float32 tensor of that layout is read in place).  Behaves
        as T x (set_actions(actions[t]); step()), with auto_reset as T x (...; reset_done(seed)); the fields hold the
        state after T steps and the outputs of the last one.  log=True also returns the per-step `reward` (T, N) int8 and
        `done` (T, N) uint8, returns=True the per-env sum of the call's rewards `returns` (N,) float32 -- device tensors
        in a dict (None when neither is asked for).  dry_run=True evaluates only: nothing resident changes.
        On torch's stream (use_torch_stream) the call is ordered with the torch ops around it and waits for nothing;
        on the engine's own stream it waits for torch's current stream before and for its own launch after."""
        import torch
        if auto_reset and dry_run:
            raise ValueError("dry_run and auto_reset exclude each other: the re-arm writes the return ring")
        tape, ld = self._tape_tensor(actions, layout)
        T, n = int(tape.shape[0]), self.n_envs
        dev = tape.device
        out = {}
        if log:
            out["reward"] = torch.empty((T, n), dtype=torch.int8, device=dev)
            out["done"] = torch.empty((T, n), dtype=torch.uint8, device=dev)
        if returns:
            out["returns"] = torch.zeros(n, dtype=torch.float32, device=dev)
        arg = L.MtTape()
        arg.struct_size = C.sizeof(L.MtTape)
        arg.n_steps = T
        arg.actions = tape.data_ptr() if T else None
        arg.ld = ld
        arg.reward_log = out["reward"].data_ptr() if log and T else None
        arg.done_log = out["done"].data_ptr() if log and T else None
        arg.log_ld = n
        arg.return_out = out["returns"].data_ptr() if returns else None
        arg.seed = int(seed)
        arg.flags = (L.TAPE_AUTO_RESET if auto_reset else 0) | (L.TAPE_DRY_RUN if dry_run else 0)
        arg.reserved = 0
        self._torch_call(self._lib.mt_rollout_tape, C.byref(arg), commits=not dry_run)
        return out or None

    _ACTIVATIONS = {"identity": L.ACT_IDENTITY, "tanh": L.ACT_TANH, "relu": L.ACT_RELU}

    @staticmethod
    def _policy_layers(layers, hidden, out):
        """[(weight, bias), ...] of a policy given as such a list or as a torch.nn.Sequential of Linear / Tanh / ReLU, whose
        activations must then be the one `hidden` and the one `out` of the call."""
        import torch
        if not isinstance(layers, torch.nn.Sequential):
            return [tuple(pair) for pair in layers]
        names = {torch.nn.Tanh: "tanh", torch.nn.ReLU: "relu"}
        pairs, acts = [], []
        for m in layers:
            if isinstance(m, torch.nn.Linear):
                if m.bias is None:
                    raise ValueError(f"layer {len(pairs)}: a Linear without bias is not supported")
                pairs.append((m.weight, m.bias))
                acts.append("identity")
            elif type(m) in names and pairs and acts[-1] == "identity":
                acts[-1] = names[type(m)]
            else:
                raise ValueError(f"a policy module is Linear layers, each followed by at most one Tanh or ReLU; got {type(m).__name__}")
        if not pairs:
            raise ValueError("the policy has no Linear layer")
        if any(a != hidden for a in acts[:-1]) or acts[-1] != out:
            raise ValueError(f"the module's activations {acts} do not agree with hidden={hidden!r}, out={out!r}")
        return pairs

    def rollout_policy(self, layers, steps, *, hidden="tanh", out="tanh", out_scale=180.0, see_pose=False, sigma=None, draw=0,
                       seed=0x5EED, auto_reset=False, lo=-180., hi=180., log=False, returns=False, actions=False,
                       observations=False, dry_run=False, logp=False, critic=None, critic_hidden="tanh", critic_out="identity",
                       critic_out_scale=1.0):
        """`steps` steps driven by an MLP policy in ONE launch (mt_rollout_policy): at every step each env's observation at
        the state it is in (the 3K floats observe() would give; see_pose=True appends the D joint angles) goes through
        `layers` -- a list of (weight, bias) CUDA float32 tensors in torch.nn.Linear layout, read in place, or a
        torch.nn.Sequential of Linear / Tanh / ReLU -- and action = clamp(out_scale * out(y) + sigma * z, lo, hi) is
        stepped.  At most 3 layers, hidden widths up to 64; hidden in ("tanh", "relu"), out in ("tanh", "identity").
        sigma: None, a float or D floats (degrees): exploration noise from the (seed, env, draw, step) stream.  The
        state afterwards is what rollout_actions leaves for the logged actions.  Returns a dict of device tensors (None
        when nothing is asked for): log -> `reward` (T, N) int8, `done` (T, N) uint8; returns -> `returns` (N,);
        actions -> `actions` (T, D, N); observations -> `observations` (T, IN, N).  dry_run=True evaluates only.
        logp=True and / or critic= (a value head as `layers` is given, on the same input: unflatten_value's views, or a
        Sequential; critic_hidden / critic_out / critic_out_scale as values() takes them) make it the actor-critic
        collection, still ONE launch (mt_rollout_actor_critic): `logp` (T, N) is policy_eval's logp of the logged actions
        under `sigma` (every entry > 0 then), `values` (T, N) is values() of the logged observations and `last_value`
        (N,) the critic on the state behind the last step -- what gae() takes -- each bit for bit, with neither log
        needed.  A critic needs 3K + IN <= 160.  Stream behaviour as rollout_actions."""
        import torch
        if auto_reset and dry_run:
            raise ValueError("dry_run and auto_reset exclude each other: the re-arm writes the return ring")
        for name, v, allowed in (("hidden", hidden, ("tanh", "relu")), ("out", out, ("tanh", "identity"))):
            if v not in allowed:
                raise ValueError(f"{name} must be one of {allowed}, got {v!r}")
        pairs = self._policy_layers(layers, hidden, out)
        if not 1 <= len(pairs) <= L.POLICY_MAX_LAYERS:
            raise ValueError(f"a policy has 1..{L.POLICY_MAX_LAYERS} linear layers, got {len(pairs)}")
        T, n, d = int(steps), self.n_envs, self.dof
        if not 0 <= T <= 65535:
            raise ValueError(f"steps must be 0..65535, got {T}")
        dev = torch.device("cuda", self.device)
        n_in = 3 * self.obj_number + (d if see_pose else 0)
        if not (logp or critic is not None):
            arg = L.MtPolicy()
        else:
            full = L.MtActorCritic()
            arg = full.policy
        keep = []
        fan_in = n_in
        for l, (w, b) in enumerate(pairs):
            w, b = w.detach(), b.detach()
            fan_out = d if l == len(pairs) - 1 else int(w.shape[0]) if w.dim() == 2 else -1
            if tuple(w.shape) != (fan_out, fan_in) or tuple(b.shape) != (fan_out,):
                raise ValueError(f"layer {l}: weight must be ({fan_out if fan_out > 0 else 'out'}, {fan_in}) and bias (out,), got "
                                 f"{tuple(w.shape)} and {tuple(b.shape)}")
            if l < len(pairs) - 1 and not 1 <= fan_out <= L.POLICY_MAX_WIDTH:
                raise ValueError(f"layer {l}: width must be 1..{L.POLICY_MAX_WIDTH}, got {fan_out}")
            for what, t in (("weight", w), ("bias", b)):
                if t.dtype != torch.float32 or not t.is_cuda or t.device != dev or not t.is_contiguous():
                    raise ValueError(f"layer {l}: {what} must be a contiguous float32 tensor on {dev}")
            keep += [w, b]
            arg.weight[l], arg.bias[l] = w.data_ptr(), b.data_ptr()
            if l < len(pairs) - 1:
                arg.width[l] = fan_out
            fan_in = fan_out
        sig = np.zeros(L.MT_MAX_DOF, dtype=np.float32)
        if sigma is not None:
            sig[:d] = np.broadcast_to(np.asarray(sigma, dtype=np.float32), (d,))
        res = {}
        if log:
            res["reward"] = torch.empty((T, n), dtype=torch.int8, device=dev)
            res["done"] = torch.empty((T, n), dtype=torch.uint8, device=dev)
        if returns:
            res["returns"] = torch.zeros(n, dtype=torch.float32, device=dev)
        if actions:
            res["actions"] = torch.empty((T, d, n), dtype=torch.float32, device=dev)
        if observations:
            res["observations"] = torch.empty((T, n_in, n), dtype=torch.float32, device=dev)
        arg.struct_size = C.sizeof(L.MtPolicy)
        arg.n_steps, arg.n_layers = T, len(pairs)
        arg.hidden_act, arg.out_act = self._ACTIVATIONS[hidden], self._ACTIVATIONS[out]
        arg.draw = int(draw) & 0xFFFFFFFF
        arg.out_scale, arg.lo, arg.hi = float(out_scale), float(lo), float(hi)
        arg.sigma[:] = sig.tolist()
        arg.flags = ((L.POLICY_AUTO_RESET if auto_reset else 0) | (L.POLICY_DRY_RUN if dry_run else 0)
                     | (L.POLICY_SEE_POSE if see_pose else 0))
        arg.action_log = res["actions"].data_ptr() if actions and T else None
        arg.obs_log = res["observations"].data_ptr() if observations and T else None
        arg.reward_log = res["reward"].data_ptr() if log and T else None
        arg.done_log = res["done"].data_ptr() if log and T else None
        arg.act_ld = arg.obs_ld = arg.log_ld = n
        arg.return_out = res["returns"].data_ptr() if returns else None
        arg.seed = int(seed)
        arg.reserved = 0
        if not (logp or critic is not None):
            self._torch_call(self._lib.mt_rollout_policy, C.byref(arg), commits=not dry_run)
            del keep
            return res or None
        full.struct_size = C.sizeof(L.MtActorCritic)
        if logp:
            if not (np.isfinite(sig[:d]).all() and (sig[:d] > 0).all()):
                raise ValueError(f"logp needs sigma: D entries, finite and > 0, got {sigma!r}")
            res["logp"] = torch.empty((T, n), dtype=torch.float32, device=dev)
            full.logp_log, full.logp_ld = (res["logp"].data_ptr() if T else None), n
        if critic is not None:
            for name, v, allowed in (("critic_hidden", critic_hidden, ("tanh", "relu")), ("critic_out", critic_out, ("tanh", "identity"))):
                if v not in allowed:
                    raise ValueError(f"{name} must be one of {allowed}, got {v!r}")
            if not np.isfinite(np.float32(critic_out_scale)):
                raise ValueError("critic_out_scale must be finite")
            keep += self._critic_arg(full, critic, critic_hidden, critic_out, n_in)
            full.critic_out_scale = float(critic_out_scale)
            res["values"] = torch.empty((T, n), dtype=torch.float32, device=dev)
            res["last_value"] = torch.empty(n, dtype=torch.float32, device=dev)
            full.value_log, full.value_ld = (res["values"].data_ptr() if T else None), n
            full.last_value_out = res["last_value"].data_ptr() if T else None
        full.reserved = 0
        if T:                                                    # (no step: nothing to write, and no address to hand over)
            self._torch_call(self._lib.mt_rollout_actor_critic, C.byref(full), commits=not dry_run)
        del keep
        return res

    def _critic_arg(self, full, critic, hidden, out, n_in):
        """The value head of rollout_policy's `critic` into `full` (critic_layers, widths, activations, weight, bias): the
        policy's layout and limits with one output.  -> the tensors to keep alive."""
        import torch
        dev = torch.device("cuda", self.device)
        pairs = self._policy_layers(critic, hidden, out)
        if not 1 <= len(pairs) <= L.POLICY_MAX_LAYERS:
            raise ValueError(f"critic: a value head has 1..{L.POLICY_MAX_LAYERS} linear layers, got {len(pairs)}")
        keep, fan_in = [], n_in
        for l, (w, b) in enumerate(pairs):
            w, b = w.detach(), b.detach()
            fan_out = 1 if l == len(pairs) - 1 else int(w.shape[0]) if w.dim() == 2 else -1
            if tuple(w.shape) != (fan_out, fan_in) or tuple(b.shape) != (fan_out,):
                raise ValueError(f"critic layer {l}: weight must be ({fan_out if fan_out > 0 else 'out'}, {fan_in}) and bias (out,), "
                                 f"got {tuple(w.shape)} and {tuple(b.shape)}")
            if l < len(pairs) - 1 and not 1 <= fan_out <= L.POLICY_MAX_WIDTH:
                raise ValueError(f"critic layer {l}: width must be 1..{L.POLICY_MAX_WIDTH}, got {fan_out}")
            for what, t in (("weight", w), ("bias", b)):
                if t.dtype != torch.float32 or not t.is_cuda or t.device != dev or not t.is_contiguous():
                    raise ValueError(f"critic layer {l}: {what} must be a contiguous float32 tensor on {dev}")
            keep += [w, b]
            full.critic_weight[l], full.critic_bias[l] = w.data_ptr(), b.data_ptr()
            if l < len(pairs) - 1:
                full.critic_width[l] = fan_out
            fan_in = fan_out
        full.critic_layers = len(pairs)
        full.critic_hidden_act, full.critic_out_act = self._ACTIVATIONS[hidden], self._ACTIVATIONS[out]
        return keep

    # ---- evolution strategies: a population of policies, one row of flat parameters per member ----------------------------
    def _policy_shapes(self, widths, see_pose=False, n_out=None):
        """[(out, in), ...] of the linear layers of a policy with hidden `widths` on this engine; the last one has `n_out`
        outputs (None: D, a policy; a value head has 1)."""
        widths = tuple(int(w) for w in widths)
        if len(widths) > L.POLICY_MAX_LAYERS - 1 or any(not 1 <= w <= L.POLICY_MAX_WIDTH for w in widths):
            raise ValueError(f"widths must be at most {L.POLICY_MAX_LAYERS - 1} hidden widths of 1..{L.POLICY_MAX_WIDTH}, got {widths}")
        fan_in, shapes = 3 * self.obj_number + (self.dof if see_pose else 0), []
        for fan_out in widths + (self.dof if n_out is None else int(n_out),):
            shapes.append((fan_out, fan_in))
            fan_in = fan_out
        return shapes

    def policy_size(self, widths=(), see_pose=False, n_out=None) -> int:
        """P, the number of floats of a policy with hidden `widths`: sum of out * in + out over its layers (`n_out`: the
        outputs of the last one, None = D)."""
        return sum(o * i + o for o, i in self._policy_shapes(widths, see_pose, n_out))

    def value_size(self, widths=(), see_pose=False) -> int:
        """P_v, the number of floats of a value head with hidden `widths`: a policy whose last layer has one output."""
        return self.policy_size(widths, see_pose, 1)

    @staticmethod
    def flatten_policy(layers):
        """theta of a policy given as rollout_policy takes it: W0 | b0 | W1 | b1 | ... as one new float32 vector."""
        import torch
        if isinstance(layers, torch.nn.Sequential):
            pairs = [(m.weight, m.bias) for m in layers if isinstance(m, torch.nn.Linear)]
        else:
            pairs = [tuple(p) for p in layers]
        return torch.cat([t.detach().reshape(-1) for pair in pairs for t in pair]).to(torch.float32).contiguous()

    def unflatten_policy(self, theta, widths=(), see_pose=False, n_out=None):
        """[(weight, bias), ...] VIEWS of `theta` (P floats, a row of a population included): what rollout_policy accepts."""
        shapes = self._policy_shapes(widths, see_pose, n_out)
        need = sum(o * i + o for o, i in shapes)
        if theta.dim() != 1 or theta.shape[0] < need or theta.stride(0) != 1:
            raise ValueError(f"theta must be a dense vector of at least P = {need} floats, got shape {tuple(theta.shape)}")
        out, off = [], 0
        for o, i in shapes:
            out.append((theta[off:off + o * i].view(o, i), theta[off + o * i:off + o * i + o]))
            off += o * i + o
        return out

    def unflatten_value(self, theta, widths=(), see_pose=False):
        """[(weight, bias), ...] VIEWS of a value head's flat `theta` (P_v floats): what values / value_grad accept."""
        return self.unflatten_policy(theta, widths, see_pose, 1)

    def _members(self, members):
        m = int(members)
        if m < 2 or m % 2 or m > L.ES_MAX_MEMBERS:
            raise ValueError(f"members must be even (antithetic pairs), 2..{L.ES_MAX_MEMBERS}, got {members}")
        return m

    def _flat_vector(self, t, name, size=None):
        import torch
        dev = torch.device("cuda", self.device)
        if not _is_torch_tensor(t) or t.dtype != torch.float32 or t.device != dev or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous 1-d float32 tensor on {dev}")
        if size is not None and t.shape[0] != size:
            raise ValueError(f"{name} must have P = {size} elements, got {t.shape[0]}")
        return t

    def _population_tensor(self, pop, members, size, name="pop"):
        import torch
        dev = torch.device("cuda", self.device)
        if (not _is_torch_tensor(pop) or pop.dtype != torch.float32 or pop.device != dev or pop.dim() != 2
                or pop.shape[0] != members or (pop.shape[1] > 1 and pop.stride(1) != 1)):
            raise ValueError(f"{name} must be a float32 ({members}, >= P) tensor on {dev} with dense rows")
        pitch = int(pop.stride(0))
        if pop.shape[1] < size or pitch < size:
            raise ValueError(f"{name}: rows of {pop.shape[1]} floats, pitch {pitch}: smaller than P = {size}")
        return pitch

    @staticmethod
    def _positive(sigma, name="sigma"):
        s = float(np.float32(sigma))
        if not (np.isfinite(s) and s > 0.0):
            raise ValueError(f"{name} must be finite and > 0, got {sigma!r}")
        return s

    def sample_population(self, theta, sigma, *, members, draw=0, seed=0x5EED, out=None):
        """The (M, P) population es() with the same arguments scores (mt_es_sample): row 2p is theta + sigma * eps_p, row
        2p + 1 theta - sigma * eps_p, eps the library's counter-based noise keyed by (seed, pair, draw, parameter).  `theta`
        is a CUDA float32 vector read in place; `out`, if given, is a float32 (M, >= P) tensor with dense rows whose words
        past P are left alone.  Returns the population.  Stream rules as rollout_actions."""
        import torch
        m, s = self._members(members), self._positive(sigma)
        theta = self._flat_vector(theta, "theta")
        p = int(theta.shape[0])
        if p < 1:
            raise ValueError("theta is empty")
        if out is None:
            out = torch.empty((m, p), dtype=torch.float32, device=theta.device)
        pitch = self._population_tensor(out, m, p, "out")
        arg = L.MtEsSample()
        arg.struct_size = C.sizeof(L.MtEsSample)
        arg.n_members, arg.n_params = m, p
        arg.theta, arg.pop, arg.pitch = theta.data_ptr(), out.data_ptr(), pitch
        arg.sigma, arg.draw, arg.seed = s, int(draw) & 0xFFFFFFFF, int(seed)
        arg.reserved = 0
        self._torch_call(self._lib.mt_es_sample, C.byref(arg), commits=False)
        return out

    def _population_arg(self, arg, pop, members, steps, widths, hidden, out, out_scale, see_pose, seed, auto_reset, dry_run, lo, hi,
                        res, log, actions, observations):
        """Fills a struct mt_population and allocates the logs asked for into `res`; returns (M, P, T)."""
        import torch
        if auto_reset and dry_run:
            raise ValueError("dry_run and auto_reset exclude each other: the re-arm writes the return ring")
        for name, v, allowed in (("hidden", hidden, ("tanh", "relu")), ("out", out, ("tanh", "identity"))):
            if v not in allowed:
                raise ValueError(f"{name} must be one of {allowed}, got {v!r}")
        m = self._members(members)
        n, d, T = self.n_envs, self.dof, int(steps)
        if not 0 <= T <= 65535:
            raise ValueError(f"steps must be 0..65535, got {T}")
        if n % m or (n // m) % 256:
            raise ValueError(f"n_envs = {n} must be members * G with G a multiple of 256 (the rollout block), got members = {m}")
        shapes = self._policy_shapes(widths, see_pose)
        p = sum(o * i + o for o, i in shapes)
        pitch = self._population_tensor(pop, m, p)
        dev = pop.device
        if log:
            res["reward"] = torch.empty((T, n), dtype=torch.int8, device=dev)
            res["done"] = torch.empty((T, n), dtype=torch.uint8, device=dev)
        if actions:
            res["actions"] = torch.empty((T, d, n), dtype=torch.float32, device=dev)
        if observations:
            res["observations"] = torch.empty((T, shapes[0][1], n), dtype=torch.float32, device=dev)
        arg.struct_size = C.sizeof(L.MtPopulation)
        arg.n_steps, arg.n_members, arg.n_layers = T, m, len(shapes)
        for l, (o, _) in enumerate(shapes[:-1]):
            arg.width[l] = o
        arg.hidden_act, arg.out_act = self._ACTIVATIONS[hidden], self._ACTIVATIONS[out]
        arg.pop, arg.pitch = pop.data_ptr(), pitch
        arg.out_scale, arg.lo, arg.hi = float(out_scale), float(lo), float(hi)
        arg.flags = ((L.POLICY_AUTO_RESET if auto_reset else 0) | (L.POLICY_DRY_RUN if dry_run else 0)
                     | (L.POLICY_SEE_POSE if see_pose else 0))
        arg.action_log = res["actions"].data_ptr() if actions and T else None
        arg.obs_log = res["observations"].data_ptr() if observations and T else None
        arg.reward_log = res["reward"].data_ptr() if log and T else None
        arg.done_log = res["done"].data_ptr() if log and T else None
        arg.act_ld = arg.obs_ld = arg.log_ld = n
        arg.seed = int(seed)
        arg.reserved = 0
        return m, p, T

    def rollout_population(self, pop, steps, *, widths=(), hidden="tanh", out="tanh", out_scale=180.0, see_pose=False,
                           seed=0x5EED, auto_reset=False, lo=-180., hi=180., log=False, returns=False, actions=False,
                           observations=False, dry_run=False):
        """M policies scored in ONE launch (mt_rollout_population): row m of `pop` -- a CUDA float32 (M, >= P) tensor with
        dense rows, each row the flat parameters of a policy with hidden `widths` (flatten_policy's layout) -- drives the
        G = N / M envs [mG, (m+1)G) as rollout_policy would with unflatten_policy(pop[m]) as its layers, bit for bit; there
        is no action noise.  M is even and G a multiple of 256.  Returns rollout_policy's dict (log / returns / actions /
        observations) plus `fitness` (M,): each member's mean return over its envs.  The other keywords, the state
        afterwards and the stream behaviour are rollout_policy's."""
        import torch
        res = {}
        arg = L.MtPopulation()
        m, _, T = self._population_arg(arg, pop, pop.shape[0] if _is_torch_tensor(pop) and pop.dim() == 2 else 0, steps, widths, hidden,
                                       out, out_scale, see_pose, seed, auto_reset, dry_run, lo, hi, res, log, actions, observations)
        ret = torch.zeros(self.n_envs, dtype=torch.float32, device=pop.device)
        res["fitness"] = torch.zeros(m, dtype=torch.float32, device=pop.device)
        if returns:
            res["returns"] = ret
        arg.return_out, arg.fitness_out = ret.data_ptr(), res["fitness"].data_ptr()
        self._torch_call(self._lib.mt_rollout_population, C.byref(arg), commits=not dry_run and T > 0)
        return res

    def es(self, theta, sigma, *, members, steps, widths=(), shaping="rank", lr=None, inplace=False, draw=0, seed=0x5EED,
           hidden="tanh", out="tanh", out_scale=180.0, see_pose=False, auto_reset=False, dry_run=False, lo=-180., hi=180.,
           log=False, population=None, returns=None, update_only=False):
        """One generation of an antithetic evolution strategy in one call (mt_es): `members` perturbed copies of `theta`
        (sample_population's, with the same sigma / draw / seed) are scored over `steps` steps (rollout_population's, each
        member on its own N / M envs), and the gradient estimate follows from the members' integer return sums:
        shaping="rank" weighs a member by its centred mid-rank, "raw" by its return sum.  Four launches, no host wait.
        Returns a dict of device tensors: `grad` (P,), ascent direction of the mean return; `fitness` (M,); `best` (1,)
        int32, the lowest member with the largest sum; `returns` (N,); `population` (M, P); `sums` (M,) int64, the members'
        return sums, and `coeff` (M / 2,) int64, the pair weights they shape into; with log=True `reward` / `done` as rollout_policy.  inplace=True also does theta += lr * grad.
        `population` / `returns` may be given as workspaces (the population as for sample_population's `out`).
        update_only=True skips sampling and scoring and updates from `returns` as given (integer-valued floats).  The
        policy keywords, the state afterwards and the stream behaviour are rollout_population's."""
        import torch
        if shaping not in ("rank", "raw"):
            raise ValueError(f"shaping must be 'rank' or 'raw', got {shaping!r}")
        if inplace and lr is None:
            raise ValueError("inplace=True needs lr")
        if update_only and returns is None:
            raise ValueError("update_only=True needs returns")
        m, s = self._members(members), self._positive(sigma)
        p = self.policy_size(widths, see_pose)
        theta = self._flat_vector(theta, "theta", p)
        dev = theta.device
        if population is None:
            population = torch.empty((m, p), dtype=torch.float32, device=dev)
        if returns is None:
            returns = torch.zeros(self.n_envs, dtype=torch.float32, device=dev)
        elif tuple(self._flat_vector(returns, "returns").shape) != (self.n_envs,):
            raise ValueError(f"returns must have n_envs = {self.n_envs} elements")
        res = {}
        arg = L.MtEs()
        _, _, T = self._population_arg(arg.pop, population, m, steps, widths, hidden, out, out_scale, see_pose, seed, auto_reset,
                                       dry_run, lo, hi, res, log, False, False)
        res.update(grad=torch.zeros(p, dtype=torch.float32, device=dev), fitness=torch.zeros(m, dtype=torch.float32, device=dev),
                   best=torch.zeros(1, dtype=torch.int32, device=dev), returns=returns, population=population,
                   coeff=torch.zeros(m // 2 + m, dtype=torch.int64, device=dev))
        arg.pop.return_out, arg.pop.fitness_out = returns.data_ptr(), res["fitness"].data_ptr()
        arg.struct_size = C.sizeof(L.MtEs)
        arg.shaping = L.ES_SHAPE_RAW if shaping == "raw" else L.ES_SHAPE_RANK
        arg.sigma, arg.lr = s, float(lr) if lr is not None else 0.0
        arg.draw = int(draw) & 0xFFFFFFFF
        arg.flags = (L.ES_INPLACE if inplace else 0) | (L.ES_UPDATE_ONLY if update_only else 0)
        arg.theta, arg.grad_out = theta.data_ptr(), res["grad"].data_ptr()
        arg.best_out, arg.coeff_out = res["best"].data_ptr(), res["coeff"].data_ptr()
        arg.reserved = 0
        self._torch_call(self._lib.mt_es, C.byref(arg), commits=not dry_run and not update_only and T > 0)
        res["coeff"], res["sums"] = res["coeff"][:m // 2], res["coeff"][m // 2:]
        return res

    # ---- the policy's log-likelihood gradient from rollout_policy's logs ---------------------------------------------------
    def _log_rows(self, t, name, rows, dtype):
        """A (T, rows, N) log (rows None: (T, N)) as the library reads it: `dtype`, on this device, unit stride along the
        envs, whole rows of ld >= N elements between them (a [..., :N] view of a wider buffer is read in place).
        -> (T, ld)."""
        import torch
        dev = torch.device("cuda", self.device)
        shape = (rows, self.n_envs) if rows is not None else (self.n_envs,)
        if (not _is_torch_tensor(t) or t.dtype != dtype or t.device != dev or t.dim() != len(shape) + 1
                or tuple(t.shape[1:]) != shape):
            raise ValueError(f"{name} must be a {dtype} tensor of shape (T, {', '.join(str(v) for v in shape)}) on {dev}")
        T, n = int(t.shape[0]), self.n_envs
        st = [int(v) for v in t.stride()]
        if rows is None:
            ld = st[0] if T > 1 else n
            dense = True
        else:
            ld = st[1] if rows > 1 else st[0] if T > 1 else n
            dense = T <= 1 or st[0] == rows * ld
        if not (dense and ld >= n and (n == 1 or st[-1] == 1)):
            raise ValueError(f"{name}: envs must be contiguous and the rows a constant ld >= N apart, got strides {tuple(st)}")
        return T, ld

    def _policy_net_arg(self, arg, layers_or_theta, widths, hidden, out, see_pose, n_out):
        """The network of policy_grad / policy_eval / value_grad into `arg` (weight, bias, width): `layers_or_theta` is a list
        of (weight, bias), a torch.nn.Sequential, or the flat theta of flatten_policy with the hidden `widths`; the last layer
        has `n_out` outputs.  -> (tensors to keep alive, number of layers, IN, P)."""
        import torch
        for name, v, allowed in (("hidden", hidden, ("tanh", "relu")), ("out", out, ("tanh", "identity"))):
            if v not in allowed:
                raise ValueError(f"{name} must be one of {allowed}, got {v!r}")
        dev = torch.device("cuda", self.device)
        d = self.dof
        if _is_torch_tensor(layers_or_theta):
            p = self.policy_size(widths, see_pose, n_out)
            pairs = self.unflatten_policy(self._flat_vector(layers_or_theta, "theta", p), widths, see_pose, n_out)
        else:
            pairs = self._policy_layers(layers_or_theta, hidden, out)
        if not 1 <= len(pairs) <= L.POLICY_MAX_LAYERS:
            raise ValueError(f"a policy has 1..{L.POLICY_MAX_LAYERS} linear layers, got {len(pairs)}")
        n_in = 3 * self.obj_number + (d if see_pose else 0)
        keep, fan_in, p = [], n_in, 0
        for l, (w, b) in enumerate(pairs):
            w, b = w.detach(), b.detach()
            fan_out = n_out if l == len(pairs) - 1 else int(w.shape[0]) if w.dim() == 2 else -1
            if tuple(w.shape) != (fan_out, fan_in) or tuple(b.shape) != (fan_out,):
                raise ValueError(f"layer {l}: weight must be ({fan_out if fan_out > 0 else 'out'}, {fan_in}) and bias (out,), got "
                                 f"{tuple(w.shape)} and {tuple(b.shape)}")
            if l < len(pairs) - 1 and not 1 <= fan_out <= L.POLICY_MAX_WIDTH:
                raise ValueError(f"layer {l}: width must be 1..{L.POLICY_MAX_WIDTH}, got {fan_out}")
            for what, t in (("weight", w), ("bias", b)):
                if t.dtype != torch.float32 or not t.is_cuda or t.device != dev or not t.is_contiguous():
                    raise ValueError(f"layer {l}: {what} must be a contiguous float32 tensor on {dev}")
            keep += [w, b]
            arg.weight[l], arg.bias[l] = w.data_ptr(), b.data_ptr()
            if l < len(pairs) - 1:
                arg.width[l] = fan_out
            p += fan_out * fan_in + fan_out
            fan_in = fan_out
        return keep, len(pairs), n_in, p

    def reward_to_go(self, reward_log, done_log, gamma=1.0, baseline=0.0, mask_after_done=False, out=None):
        """The discounted reward-to-go of rollout_policy's logs (mt_reward_to_go): R_t = r_t + gamma * (0 if done_t else
        R_t+1), minus `baseline`, as a (T, N) float32 device tensor -- policy_grad's usual `coef`.  mask_after_done=True
        (logs WITHOUT auto_reset, where an env steps on after its episode ended) writes exactly 0 behind an env's first done:
        policy_grad skips such samples.  One launch; stream behaviour as rollout_actions."""
        import torch
        T, ld = self._log_rows(reward_log, "reward_log", None, torch.int8)
        T2, ld2 = self._log_rows(done_log, "done_log", None, torch.uint8)
        if T2 != T or (T > 1 and ld2 != ld):
            raise ValueError("reward_log and done_log must have the same shape and strides")
        g = float(np.float32(gamma))
        if not 0.0 <= g <= 1.0:
            raise ValueError(f"gamma must be in [0, 1], got {gamma!r}")
        if not np.isfinite(np.float32(baseline)):
            raise ValueError(f"baseline must be finite, got {baseline!r}")
        if out is None:
            out = torch.empty((T, self.n_envs), dtype=torch.float32, device=reward_log.device)
        To, out_ld = self._log_rows(out, "out", None, torch.float32)
        if To != T:
            raise ValueError(f"out must have T = {T} rows")
        arg = L.MtRewardToGo()
        arg.struct_size = C.sizeof(L.MtRewardToGo)
        arg.n_steps = T
        arg.reward_log, arg.done_log, arg.log_ld = (reward_log.data_ptr(), done_log.data_ptr(), ld) if T else (None, None, self.n_envs)
        arg.gamma, arg.baseline = g, float(baseline)
        arg.out, arg.out_ld = (out.data_ptr() if T else None), out_ld
        arg.flags = L.RTG_MASK_AFTER_DONE if mask_after_done else 0
        arg.reserved = 0
        self._torch_call(self._lib.mt_reward_to_go, C.byref(arg), commits=False)
        return out

    def policy_grad(self, layers_or_theta, obs, actions, coef, *, sigma, widths=(), hidden="tanh", out="tanh", out_scale=180.0,
                    see_pose=False, scale=1.0, grad_out=None, loss=False, old_logp=None, clip=0.2, weights=None, sigma_old=None,
                    ratio=False, coef_out=False, sigma_grad=False):
        """grad = scale * sum over samples (t, i) of coef[t, i] * d logp / d theta (mt_policy_grad), logp = -1/2 sum_j
        ((actions[t, j, i] - mu_j(obs[t, :, i])) / sigma_j)^2, mu the policy's action before noise and clamp -- the
        REINFORCE direction with coef = reward_to_go(...), behaviour cloning with coef = 1, sigma = 1.  `layers_or_theta`: a
        list of (weight, bias), a torch.nn.Sequential (both as rollout_policy takes them), or the flat theta of
        flatten_policy with the hidden `widths`.  obs (T, IN, N), actions (T, D, N), coef (T, N): float32 device tensors
        as rollout_policy(observations=True, actions=True) returns them, or [..., :N] views of wider buffers.  sigma: a
        float or D floats, > 0.  A sample with coef == 0 or an unusable action contributes exactly nothing.  Returns grad
        (P,) float32 in flatten_policy's layout (written into `grad_out` when given), so theta += lr * grad ascends; with
        loss=True (grad, loss), loss a (1,) tensor holding scale * sum coef * logp.  Deterministic: the same arguments give
        the same bits.  Two launches, no host wait; the workspace is cached on the engine.  Stream behaviour as
        rollout_actions; nothing resident is read or written.

        With old_logp= (T, N), policy_eval's logp when the actions were taken, the call is PPO's clipped surrogate in one
        pass (mt_ppo_grad): the positional `coef` holds the ADVANTAGES, `weights` (T, N) or None multiplies them (gae's
        `weights`), ratio = exp(logp_now - old_logp) is formed in the kernel and a sample counts with ratio * advantage
        unless it is clipped (advantage > 0 and ratio > 1 + clip, or advantage < 0 and ratio < 1 - clip); clip=0 never
        clips.  sigma_old: the sigma old_logp was taken with, when it differs from `sigma` (the dropped normalisers then
        enter the ratio).  Returns a dict of device tensors, no host sync: `grad` (P,), `loss` (1,) = scale * sum of
        min(ratio A, clamp(ratio) A), `kl` (1,) = scale * sum of (ratio - 1) - log ratio, `used` and `clipped` (int64
        scalars: the samples that count and, of them, the clipped ones) and, on request, `ratio` and `coef` (T, N; ratio=True
        / coef_out=True, or tensors to write into) and `sigma_grad` (D,) = scale * sum of coef * d logp / d log sigma_j
        (sigma_grad=True).  grad is bit for bit policy_grad(coef=that `coef`)."""
        if old_logp is not None:
            return self._ppo_grad(layers_or_theta, obs, actions, coef, old_logp, sigma=sigma, widths=widths, hidden=hidden, out=out,
                                  out_scale=out_scale, see_pose=see_pose, scale=scale, grad_out=grad_out, clip=clip, weights=weights,
                                  sigma_old=sigma_old, ratio=ratio, coef_out=coef_out, sigma_grad=sigma_grad)
        import torch
        dev = torch.device("cuda", self.device)
        d = self.dof
        arg = L.MtPolicyGrad()
        keep, n_layers, n_in, p = self._policy_net_arg(arg, layers_or_theta, widths, hidden, out, see_pose, d)
        sig = np.ones(L.MT_MAX_DOF, dtype=np.float32)
        sig[:d] = np.broadcast_to(np.asarray(sigma, dtype=np.float32), (d,))
        if not (np.isfinite(sig).all() and (sig > 0).all()):
            raise ValueError(f"sigma must be finite and > 0, got {sigma!r}")
        if not (np.isfinite(np.float32(scale)) and np.isfinite(np.float32(out_scale))):
            raise ValueError("scale and out_scale must be finite")
        T, obs_ld = self._log_rows(obs, "obs", n_in, torch.float32)
        Ta, act_ld = self._log_rows(actions, "actions", d, torch.float32)
        Tc, coef_ld = self._log_rows(coef, "coef", None, torch.float32)
        if not T == Ta == Tc:
            raise ValueError(f"obs, actions and coef must have the same number of steps, got {T}, {Ta}, {Tc}")
        if grad_out is None:
            grad_out = torch.empty(p, dtype=torch.float32, device=dev)
        else:
            self._flat_vector(grad_out, "grad_out", p)
        loss_t = torch.zeros(1, dtype=torch.float32, device=dev) if loss else None
        arg.struct_size = C.sizeof(L.MtPolicyGrad)
        arg.n_steps, arg.n_layers = T, n_layers
        arg.hidden_act, arg.out_act = self._ACTIVATIONS[hidden], self._ACTIVATIONS[out]
        arg.out_scale, arg.scale = float(out_scale), float(scale)
        arg.sigma[:] = sig.tolist()
        arg.flags = L.POLICY_SEE_POSE if see_pose else 0
        arg.obs, arg.action, arg.coef = (obs.data_ptr(), actions.data_ptr(), coef.data_ptr()) if T else (None, None, None)
        arg.obs_ld, arg.act_ld, arg.coef_ld = obs_ld, act_ld, coef_ld
        arg.grad_out = grad_out.data_ptr()
        arg.loss_out = loss_t.data_ptr() if loss else None
        need = int(self._lib.mt_policy_grad_workspace(self._h, n_layers, arg.width, arg.flags, T))
        ws = getattr(self, "_pg_workspace", None)
        if need and (ws is None or ws.numel() * 4 < need):
            ws = self._pg_workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
        arg.workspace = ws.data_ptr() if need else None
        arg.workspace_bytes = ws.numel() * 4 if need else 0
        arg.reserved = 0
        self._torch_call(self._lib.mt_policy_grad, C.byref(arg), commits=False)
        del keep
        return (grad_out, loss_t) if loss else grad_out

    def _ppo_grad(self, layers_or_theta, obs, actions, adv, old_logp, *, sigma, widths, hidden, out, out_scale, see_pose, scale,
                  grad_out, clip, weights, sigma_old, ratio, coef_out, sigma_grad):
        """policy_grad(..., old_logp=): mt_ppo_grad."""
        import torch
        dev = torch.device("cuda", self.device)
        d, n = self.dof, self.n_envs
        arg = L.MtPpoGrad()
        keep, n_layers, n_in, p = self._policy_net_arg(arg, layers_or_theta, widths, hidden, out, see_pose, d)
        sig = np.ones(L.MT_MAX_DOF, dtype=np.float32)
        sig[:d] = np.broadcast_to(np.asarray(sigma, dtype=np.float32), (d,))
        if not (np.isfinite(sig).all() and (sig > 0).all()):
            raise ValueError(f"sigma must be finite and > 0, got {sigma!r}")
        shift = 0.0
        if sigma_old is not None:
            old = np.broadcast_to(np.asarray(sigma_old, dtype=np.float32), (d,)).astype(np.float64)
            if not (np.isfinite(old).all() and (old > 0).all()):
                raise ValueError(f"sigma_old must be finite and > 0, got {sigma_old!r}")
            shift = float(np.log(old / sig[:d].astype(np.float64)).sum())
        if not (np.isfinite(np.float32(scale)) and np.isfinite(np.float32(out_scale)) and np.isfinite(np.float32(shift))):
            raise ValueError("scale, out_scale and the shift of sigma_old must be finite")
        clip = float(np.float32(clip))
        if not (clip == 0.0 or 0.0 < clip < 1.0):
            raise ValueError(f"clip must be 0 (no clipping) or in (0, 1), got {clip!r}")
        T, obs_ld = self._log_rows(obs, "obs", n_in, torch.float32)
        Ta, act_ld = self._log_rows(actions, "actions", d, torch.float32)
        Tc, adv_ld = self._log_rows(adv, "coef", None, torch.float32)
        To, old_ld = self._log_rows(old_logp, "old_logp", None, torch.float32)
        Tw, weight_ld = self._log_rows(weights, "weights", None, torch.float32) if weights is not None else (T, n)
        if not T == Ta == Tc == To == Tw:
            raise ValueError(f"obs, actions, coef, old_logp and weights must have the same number of steps, got {T}, {Ta}, {Tc}, {To}, {Tw}")
        if grad_out is None:
            grad_out = torch.empty(p, dtype=torch.float32, device=dev)
        else:
            self._flat_vector(grad_out, "grad_out", p)
        small = torch.zeros(2, dtype=torch.float32, device=dev)         # loss, kl
        count = torch.zeros(2, dtype=torch.int64, device=dev)           # used, clipped
        res = {"grad": grad_out, "loss": small[0:1], "kl": small[1:2], "used": count[0], "clipped": count[1]}
        arg.struct_size = C.sizeof(L.MtPpoGrad)
        arg.n_steps, arg.n_layers = T, n_layers
        arg.hidden_act, arg.out_act = self._ACTIVATIONS[hidden], self._ACTIVATIONS[out]
        arg.out_scale, arg.scale = float(out_scale), float(scale)
        arg.clip, arg.log_ratio_shift = clip, shift
        arg.sigma[:] = sig.tolist()
        arg.flags = L.POLICY_SEE_POSE if see_pose else 0
        arg.obs, arg.action, arg.adv, arg.old_logp = ((obs.data_ptr(), actions.data_ptr(), adv.data_ptr(), old_logp.data_ptr()) if T
                                                      else (None, None, None, None))
        arg.sample_weight = weights.data_ptr() if weights is not None and T else None
        arg.obs_ld, arg.act_ld, arg.adv_ld, arg.old_ld, arg.weight_ld = obs_ld, act_ld, adv_ld, old_ld, weight_ld
        for key, want, name, field, ld_field in (("ratio", ratio, "ratio", "ratio_out", "ratio_ld"),
                                                 ("coef", coef_out, "coef_out", "coef_out", "coef_ld")):
            given = _is_torch_tensor(want)
            if not (given or want):
                continue
            res[key] = want if given else torch.empty((T, n), dtype=torch.float32, device=dev)
            To, ld = self._log_rows(res[key], name, None, torch.float32)
            if To != T:
                raise ValueError(f"{name} must have T = {T} rows")
            setattr(arg, field, res[key].data_ptr() if T else None)
            setattr(arg, ld_field, ld)
        if sigma_grad:
            res["sigma_grad"] = torch.zeros(d, dtype=torch.float32, device=dev)
            arg.sigma_grad_out = res["sigma_grad"].data_ptr()
        arg.grad_out = grad_out.data_ptr()
        arg.loss_out, arg.kl_out, arg.count_out = res["loss"].data_ptr(), res["kl"].data_ptr(), count.data_ptr()
        need = int(self._lib.mt_ppo_grad_workspace(self._h, n_layers, arg.width, arg.flags, T))
        ws = getattr(self, "_ppo_workspace", None)
        if need and (ws is None or ws.numel() * 4 < need):
            ws = self._ppo_workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
        arg.workspace = ws.data_ptr() if need else None
        arg.workspace_bytes = ws.numel() * 4 if need else 0
        arg.reserved = 0
        self._torch_call(self._lib.mt_ppo_grad, C.byref(arg), commits=False)
        del keep
        return res

    # ---- a critic and GAE weights: the forward pass over the logs, the advantages, the value head's gradient ---------------
    def policy_eval(self, layers_or_theta, obs, *, actions=None, sigma=None, n_out=None, widths=(), hidden="tanh", out="tanh",
                    out_scale=180.0, see_pose=False, mean=True, logp=None):
        """The MLP's forward pass over logged observations (mt_policy_eval): `mean` (T, n_out, N), mu = out_scale *
        out(y_L) for every sample, bit for bit what rollout_policy and policy_grad compute for that x, and -- with `actions`
        (T, n_out, N) and `sigma` (a float or n_out floats, > 0) -- `logp` (T, N), -1/2 sum_j ((a_j - mu_j) / sigma_j)^2 in
        policy_grad's own fp32 sequence; a sample with an unusable action gets logp exactly 0.  n_out: the outputs of the
        last layer (None = D, a policy; a value head has 1).  logp=None means "when actions are given"; mean=False skips
        the mean; either may be a tensor to write into (a [..., :N] view of a wider buffer included).  The network, obs and the views accepted are policy_grad's.  Returns a dict of float32 device tensors.
        One launch, no host wait; stream behaviour as rollout_actions; nothing resident is read or written."""
        import torch
        dev = torch.device("cuda", self.device)
        no = self.dof if n_out is None else int(n_out)
        if not 1 <= no <= L.MT_MAX_DOF:
            raise ValueError(f"n_out must be 1..{L.MT_MAX_DOF}, got {n_out!r}")
        mean_given, logp_given = _is_torch_tensor(mean), _is_torch_tensor(logp)
        logp = actions is not None if logp is None else logp
        if (logp_given or logp) and (actions is None or sigma is None):
            raise ValueError("logp needs actions and sigma")
        if not (mean_given or mean or logp_given or logp):
            raise ValueError("nothing to compute: mean=False and no logp")
        arg = L.MtPolicyEval()
        keep, n_layers, n_in, _ = self._policy_net_arg(arg, layers_or_theta, widths, hidden, out, see_pose, no)
        if not np.isfinite(np.float32(out_scale)):
            raise ValueError("out_scale must be finite")
        T, obs_ld = self._log_rows(obs, "obs", n_in, torch.float32)
        res = {}
        arg.struct_size = C.sizeof(L.MtPolicyEval)
        arg.n_steps, arg.n_layers, arg.n_out = T, n_layers, no
        arg.hidden_act, arg.out_act = self._ACTIVATIONS[hidden], self._ACTIVATIONS[out]
        arg.out_scale = float(out_scale)
        arg.flags = L.POLICY_SEE_POSE if see_pose else 0
        arg.obs, arg.obs_ld = (obs.data_ptr() if T else None), obs_ld
        if mean_given or mean:
            res["mean"] = mean if mean_given else torch.empty((T, no, self.n_envs), dtype=torch.float32, device=dev)
            Tm, arg.mean_ld = self._log_rows(res["mean"], "mean", no, torch.float32)
            if Tm != T:
                raise ValueError(f"mean must have T = {T} steps")
            arg.mean_out = res["mean"].data_ptr()
        if logp_given or logp:
            sig = np.ones(L.MT_MAX_DOF, dtype=np.float32)
            sig[:no] = np.broadcast_to(np.asarray(sigma, dtype=np.float32), (no,))
            if not (np.isfinite(sig).all() and (sig > 0).all()):
                raise ValueError(f"sigma must be finite and > 0, got {sigma!r}")
            Ta, act_ld = self._log_rows(actions, "actions", no, torch.float32)
            if Ta != T:
                raise ValueError(f"obs and actions must have the same number of steps, got {T}, {Ta}")
            arg.sigma[:] = sig.tolist()
            arg.action, arg.act_ld = (actions.data_ptr() if T else None), act_ld
            res["logp"] = logp if logp_given else torch.empty((T, self.n_envs), dtype=torch.float32, device=dev)
            Tl, arg.logp_ld = self._log_rows(res["logp"], "logp", None, torch.float32)
            if Tl != T:
                raise ValueError(f"logp must have T = {T} rows")
            arg.logp_out = res["logp"].data_ptr()
        arg.reserved = 0
        if T:                                                    # (no step: nothing to write, and no address to hand over)
            self._torch_call(self._lib.mt_policy_eval, C.byref(arg), commits=False)
        del keep
        return res

    def values(self, layers_or_theta, obs, *, widths=(), hidden="tanh", out="identity", out_scale=1.0, see_pose=False):
        """V (T, N) of a value head -- an MLP of the policy's shape whose last layer has one output -- over logged
        observations: policy_eval(..., n_out=1)'s mean without its middle axis."""
        return self.policy_eval(layers_or_theta, obs, n_out=1, widths=widths, hidden=hidden, out=out, out_scale=out_scale,
                                see_pose=see_pose)["mean"][:, 0]

    def gae(self, reward_log, done_log, values, last_value=None, gamma=0.99, lam=0.95, mask_after_done=False, returns=True,
            weights=False):
        """Generalised advantage estimation (mt_gae) from rollout_policy's logs and a critic's `values` (T, N):
        delta_t = r_t + gamma * (0 if done_t else V_t+1) - V_t, A_t = delta_t + gamma * lam * (0 if done_t else A_t+1),
        V_T = `last_value` (N,) or 0.  Returns a dict of (T, N) float32 device tensors: `advantages`; with returns=True
        `returns` = A + V, the critic's regression targets; with weights=True `weights`, 1 for every step that counts.
        mask_after_done=True (logs WITHOUT auto_reset) writes exactly 0 into all three behind an env's first done, so
        `weights` is the coef that takes those steps out of value_grad.  One launch; stream behaviour as rollout_actions."""
        import torch
        T, ld = self._log_rows(reward_log, "reward_log", None, torch.int8)
        T2, ld2 = self._log_rows(done_log, "done_log", None, torch.uint8)
        if T2 != T or (T > 1 and ld2 != ld):
            raise ValueError("reward_log and done_log must have the same shape and strides")
        Tv, value_ld = self._log_rows(values, "values", None, torch.float32)
        if Tv != T:
            raise ValueError(f"values must have T = {T} rows")
        g, lm = float(np.float32(gamma)), float(np.float32(lam))
        if not (0.0 <= g <= 1.0 and 0.0 <= lm <= 1.0):
            raise ValueError(f"gamma and lam must be in [0, 1], got {gamma!r}, {lam!r}")
        dev = reward_log.device
        if last_value is not None and tuple(self._flat_vector(last_value, "last_value").shape) != (self.n_envs,):
            raise ValueError(f"last_value must have n_envs = {self.n_envs} elements")
        names = ["advantages"] + (["returns"] if returns else []) + (["weights"] if weights else [])
        res = {k: torch.empty((T, self.n_envs), dtype=torch.float32, device=dev) for k in names}
        arg = L.MtGae()
        arg.struct_size = C.sizeof(L.MtGae)
        arg.n_steps = T
        arg.reward_log, arg.done_log, arg.log_ld = (reward_log.data_ptr(), done_log.data_ptr(), ld) if T else (None, None, self.n_envs)
        arg.value, arg.value_ld = (values.data_ptr() if T else None), value_ld
        arg.last_value = last_value.data_ptr() if last_value is not None else None
        arg.gamma, arg.lambda_ = g, lm
        arg.adv_out, arg.adv_ld = (res["advantages"].data_ptr() if T else None), self.n_envs
        arg.ret_out, arg.ret_ld = (res["returns"].data_ptr() if returns and T else None), self.n_envs
        arg.weight_out, arg.weight_ld = (res["weights"].data_ptr() if weights and T else None), self.n_envs
        arg.flags = L.GAE_MASK_AFTER_DONE if mask_after_done else 0
        arg.reserved = 0
        self._torch_call(self._lib.mt_gae, C.byref(arg), commits=False)
        return res

    def value_grad(self, layers_or_theta, obs, targets, coef=None, *, widths=(), hidden="tanh", out="identity", out_scale=1.0,
                   see_pose=False, scale=1.0, grad_out=None, loss=False):
        """The critic's regression gradient (mt_value_grad, on policy_grad's kernels): grad = scale * sum over samples of
        coef[t, i] * (targets[t, i] - V) * dV / dtheta for the value head `layers_or_theta` (values' network), so theta +=
        lr * grad DESCENDS the squared error; with loss=True (grad, loss), loss = scale * sum coef * (-1/2 (R - V)^2).
        targets, coef: (T, N) float32 device tensors (gae's `returns` and `weights`); coef=None weighs every sample by 1.
        A sample with coef == 0 or an unusable target (NaN, inf, beyond +-32768) contributes exactly nothing.  Returns grad
        (P_v,) in flatten_policy's layout (written into `grad_out` when given).  Deterministic; two launches, no host wait;
        the workspace is cached on the engine, apart from policy_grad's.  Stream behaviour as rollout_actions."""
        import torch
        dev = torch.device("cuda", self.device)
        arg = L.MtValueGrad()
        keep, n_layers, n_in, p = self._policy_net_arg(arg, layers_or_theta, widths, hidden, out, see_pose, 1)
        if not (np.isfinite(np.float32(scale)) and np.isfinite(np.float32(out_scale))):
            raise ValueError("scale and out_scale must be finite")
        T, obs_ld = self._log_rows(obs, "obs", n_in, torch.float32)
        Tt, target_ld = self._log_rows(targets, "targets", None, torch.float32)
        if coef is None:
            coef = torch.ones((T, self.n_envs), dtype=torch.float32, device=dev)
        Tc, coef_ld = self._log_rows(coef, "coef", None, torch.float32)
        if not T == Tt == Tc:
            raise ValueError(f"obs, targets and coef must have the same number of steps, got {T}, {Tt}, {Tc}")
        if grad_out is None:
            grad_out = torch.empty(p, dtype=torch.float32, device=dev)
        else:
            self._flat_vector(grad_out, "grad_out", p)
        loss_t = torch.zeros(1, dtype=torch.float32, device=dev) if loss else None
        arg.struct_size = C.sizeof(L.MtValueGrad)
        arg.n_steps, arg.n_layers = T, n_layers
        arg.hidden_act, arg.out_act = self._ACTIVATIONS[hidden], self._ACTIVATIONS[out]
        arg.out_scale, arg.scale = float(out_scale), float(scale)
        arg.flags = L.POLICY_SEE_POSE if see_pose else 0
        arg.obs, arg.target, arg.coef = (obs.data_ptr(), targets.data_ptr(), coef.data_ptr()) if T else (None, None, None)
        arg.obs_ld, arg.target_ld, arg.coef_ld = obs_ld, target_ld, coef_ld
        arg.grad_out = grad_out.data_ptr()
        arg.loss_out = loss_t.data_ptr() if loss else None
        need = int(self._lib.mt_value_grad_workspace(self._h, n_layers, arg.width, arg.flags, T))
        ws = getattr(self, "_vg_workspace", None)
        if need and (ws is None or ws.numel() * 4 < need):
            ws = self._vg_workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
        arg.workspace = ws.data_ptr() if need else None
        arg.workspace_bytes = ws.numel() * 4 if need else 0
        arg.reserved = 0
        self._torch_call(self._lib.mt_value_grad, C.byref(arg), commits=False)
        del keep
        return (grad_out, loss_t) if loss else grad_out

    def shoot(self, plans, *, layout="soa", commit=0, auto_reset=False, seed=0x5EED, all_returns=False, log=False,
              returns=False):
        """A sampling planner's round in one call (mt_shoot): `plans` holds C candidate tapes of T steps per env, (C, T, D, N)
        degrees (layout="soa"; a CUDA float32 tensor with unit env stride, a uniform row pitch >= N and a uniform candidate
        stride is read in place) or (C, T, N, D) (layout="env_major", copied).  Every candidate is scored from the current
        state exactly as rollout_actions(plans[c], dry_run=True, returns=True) scores it; `best` (N,) int32 names each env's
        best one (the lowest index on a tie, numpy's argmax), `best_return` (N,) float32 its return.  commit=H > 0 then
        executes steps 0..H-1 of each env's best plan for real, as rollout_actions(gathered[:H], auto_reset=, seed=) would.
        all_returns=True adds `candidate_returns` (C, N); with a commit, log=True adds the committed steps' `reward` (H, N)
        int8 and `done` (H, N) uint8 and returns=True their per-env sum `returns` (N,).  Device tensors in a dict.
        Stream rules as rollout_actions; with commit == 0 nothing resident changes."""
        import torch
        commit = self._commit_steps(commit, auto_reset)
        tape, ld, cand_stride = self._tape_tensor(plans, layout, candidates=True)
        c, T, n = int(tape.shape[0]), int(tape.shape[1]), self.n_envs
        if not 1 <= c <= 64:
            raise ValueError(f"plans must hold 1..64 candidates, got {c}")
        dev = tape.device
        alloc = torch.empty if T else torch.zeros                # (T == 0: the call is a no-op and writes nothing)
        out = {"best": alloc(n, dtype=torch.int32, device=dev), "best_return": alloc(n, dtype=torch.float32, device=dev)}
        if all_returns:
            out["candidate_returns"] = alloc((c, n), dtype=torch.float32, device=dev)
        arg = L.MtShoot()
        arg.struct_size = C.sizeof(L.MtShoot)
        self._commit_outputs(arg, out, T, commit, log, returns, chosen=False)
        arg.n_steps, arg.n_candidates = T, c
        arg.actions = tape.data_ptr() if T else None
        arg.ld, arg.cand_stride = ld, cand_stride
        arg.returns_out = out["candidate_returns"].data_ptr() if all_returns else None
        arg.ret_ld = n
        arg.best_out = out["best"].data_ptr()
        arg.best_return_out = out["best_return"].data_ptr()
        arg.seed = int(seed)
        arg.flags = L.SHOOT_AUTO_RESET if auto_reset else 0
        arg.reserved = 0
        self._torch_call(self._lib.mt_shoot, C.byref(arg), commits=bool(commit and T))
        return out

    def _cem_rows(self, mean, sigma):
        """(mean, sigma, T, ld) of mt_cem's inputs: CUDA float32 (T, D, N) tensors on the engine's device with unit env
        stride and ONE uniform row pitch >= N, read in place.  Nothing is copied: the refit may be written onto them."""
        import torch
        n, d = self.n_envs, self.dof
        dev = torch.device("cuda", self.device)
        for name, t in (("mean", mean), ("sigma", sigma)):
            if not _is_torch_tensor(t) or not t.is_cuda or t.device != dev or t.dtype != torch.float32:
                raise ValueError(f"{name} must be a CUDA float32 tensor on the engine's device")
            if t.dim() != 3 or tuple(t.shape[1:]) != (d, n):
                raise ValueError(f"{name} must be (T, {d}, {n}), got {tuple(t.shape)}")
        if mean.shape[0] != sigma.shape[0]:
            raise ValueError("mean and sigma must cover the same number of steps")
        T = int(mean.shape[0])
        if T > 65535:
            raise ValueError(f"at most 65535 steps, got {T}")
        if T == 0:
            return mean, sigma, 0, n
        ld = int(mean.stride(1))
        for name, t in (("mean", mean), ("sigma", sigma)):
            if t.stride(2) != 1 or t.stride(1) != ld or ld < n or t.stride(0) != d * ld:
                raise ValueError(f"{name} must have unit env stride and the row pitch of mean (>= N), rows (t, j) in order")
        return mean, sigma, T, ld

    @staticmethod
    def _cem_scalars(candidates, lo, hi):
        c, lo, hi = int(candidates), float(lo), float(hi)
        if not 1 <= c <= 64:
            raise ValueError(f"candidates must be 1..64, got {c}")
        if not (np.isfinite(lo) and np.isfinite(hi) and -32768.0 <= lo <= hi <= 32768.0):
            raise ValueError(f"lo <= hi must be finite and within +-32768 degrees, got {lo}, {hi}")
        return c, lo, hi

    def sample_plans(self, mean, sigma, *, candidates, draw=0, seed=0x5EED, lo=-180., hi=180., keep_mean=False):
        """The (C, T, D, N) float32 block of candidate plans that cem() with the same arguments scores (mt_sample_plans):
        x = mean + sigma * z, clamped to [lo, hi], z the library's counter-based noise keyed by (seed, global env id, draw,
        candidate, step, joint).  `mean` and `sigma` are CUDA float32 (T, D, N) tensors read in place.  Stream rules as
        shoot()."""
        import torch
        c, lo, hi = self._cem_scalars(candidates, lo, hi)
        mean, sigma, T, ld = self._cem_rows(mean, sigma)
        n, d = self.n_envs, self.dof
        out = torch.empty((c, T, d, n), dtype=torch.float32, device=mean.device)
        arg = L.MtCem()
        arg.struct_size = C.sizeof(L.MtCem)
        arg.n_steps, arg.n_candidates, arg.draw = T, c, int(draw) & 0xFFFFFFFF
        arg.mean, arg.sigma, arg.ld = (mean.data_ptr(), sigma.data_ptr(), ld) if T else (None, None, n)
        arg.lo, arg.hi = lo, hi
        arg.seed = int(seed)
        arg.flags = L.CEM_KEEP_MEAN if keep_mean else 0
        self._torch_call(self._lib.mt_sample_plans, C.byref(arg), C.c_void_p(out.data_ptr() if T else None), C.c_int64(n),
                         C.c_int64(T * d * n), commits=False)
        return out

    def cem(self, mean, sigma, *, candidates, elites, draw=0, seed=0x5EED, commit=0, auto_reset=False, lo=-180., hi=180.,
            sigma_min=0., keep_mean=False, inplace=False, all_returns=False, elite_mask=False, log=False, returns=False):
        """One iteration of the cross-entropy method in one call (mt_cem): C = `candidates` plans per env are DRAWN in the
        kernel around `mean` / `sigma` (CUDA float32 (T, D, N), read in place; the block is what sample_plans() returns for
        the same arguments, but it never exists), scored exactly as shoot() scores them, and (mean, sigma) are refitted from
        each env's E = `elites` best (return descending, index ascending).  Returns a dict of device tensors: `best` (N,)
        int32, `best_return` (N,) float32, `mean` / `sigma` (T, D, N) -- new tensors, or with inplace=True the arguments
        themselves, overwritten -- plus `candidate_returns` (C, N) with all_returns=True and `elite_mask` (N,) int64 (bit c
        = candidate c is an elite) with elite_mask=True.  commit=H > 0 also executes steps 0..H-1 of each env's best plan
        for real, as rollout_actions(chosen, layout="soa", auto_reset=, seed=) would: `chosen` (H, D, N) holds those
        angles, log=True adds `reward` / `done` (H, N) and returns=True `returns` (N,).  sigma is floored at sigma_min;
        keep_mean=True makes candidate 0 the clamped mean.  Stream rules as shoot(); with commit == 0 nothing resident
        changes."""
        import torch
        commit = self._commit_steps(commit, auto_reset)
        c, lo, hi = self._cem_scalars(candidates, lo, hi)
        e = int(elites)
        if not 1 <= e <= c:
            raise ValueError(f"elites must be 1..candidates = {c}, got {e}")
        arg = L.MtCem()
        arg.struct_size = C.sizeof(L.MtCem)
        out, T, alloc = self._refit_args(arg, mean, sigma, c, lo, hi, sigma_min, draw, seed, inplace, True, all_returns)
        if elite_mask:
            out["elite_mask"] = alloc(self.n_envs, dtype=torch.int64)
        self._commit_outputs(arg, out, T, commit, log, returns)
        arg.n_elites = e
        arg.elite_mask_out = out["elite_mask"].data_ptr() if elite_mask else None
        arg.flags = (L.CEM_AUTO_RESET if auto_reset else 0) | (L.CEM_KEEP_MEAN if keep_mean else 0)
        arg.reserved = 0
        self._torch_call(self._lib.mt_cem, C.byref(arg), commits=bool(commit and T))
        return out

    def mppi(self, mean, sigma, *, candidates, temperature=None, decay=None, draw=0, seed=0x5EED, commit=0, auto_reset=False,
             lo=-180., hi=180., sigma_min=0., keep_mean=False, fit_sigma=False, inplace=False, all_returns=False,
             weights=False, log=False, returns=False):
        """One MPPI iteration in one call (mt_mppi): C = `candidates` plans per env are DRAWN in the kernel around `mean` /
        `sigma` exactly as cem() draws them (the block is what sample_plans() returns for the same arguments, but it never
        exists) and scored exactly as shoot() scores them; candidate c then weighs decay ** (best_return - its return) --
        give exactly one of `temperature` (lambda > 0: decay = float32(exp(-1 / lambda))) and `decay` (0 <= decay <= 1; 0
        is the hard maximum, 1 the plain average) -- and `mean` becomes the weighted mean of all candidates, with
        fit_sigma=True `sigma` their weighted standard deviation, floored at sigma_min.  Returns a dict of device tensors:
        `best` (N,) int32, `best_return` (N,) float32, `weight_sum` (N,) float32, `mean` (T, D, N) -- a new tensor, or with
        inplace=True the argument itself, overwritten -- and with fit_sigma `sigma` likewise; `candidate_returns` (C, N)
        with all_returns=True, `weights` (C, N) with weights=True.  commit=H > 0 also executes steps 0..H-1 of each env's
        best plan for real, as rollout_actions(chosen, layout="soa", auto_reset=, seed=) would: `chosen` (H, D, N) holds
        those angles, log=True adds `reward` / `done` (H, N) and returns=True `returns` (N,).  At most 127 steps.  Stream
        rules as cem(); with commit == 0 nothing resident changes."""
        import torch
        commit = self._commit_steps(commit, auto_reset)
        c, lo, hi = self._cem_scalars(candidates, lo, hi)
        if (temperature is None) == (decay is None):
            raise ValueError("give exactly one of temperature and decay")
        if temperature is not None:
            lam = float(temperature)
            if not (np.isfinite(lam) and lam > 0.0):
                raise ValueError(f"temperature must be finite and > 0, got {lam}")
            rho = float(np.float32(np.exp(-1.0 / lam)))
        else:
            rho = float(decay)
            if not (np.isfinite(rho) and 0.0 <= rho <= 1.0):
                raise ValueError(f"decay must be finite and within 0..1, got {rho}")
            rho = float(np.float32(rho))
        arg = L.MtMppi()
        arg.struct_size = C.sizeof(L.MtMppi)
        out, T, alloc = self._refit_args(arg, mean, sigma, c, lo, hi, sigma_min, draw, seed, inplace, fit_sigma, all_returns,
                                         max_steps=L.MPPI_MAX_STEPS)
        n = self.n_envs
        out["weight_sum"] = alloc(n, dtype=torch.float32)
        if weights:
            out["weights"] = alloc((c, n), dtype=torch.float32)
        self._commit_outputs(arg, out, T, commit, log, returns)
        arg.decay = rho
        arg.weights_out = out["weights"].data_ptr() if weights else None
        arg.w_ld = n
        arg.weight_sum_out = out["weight_sum"].data_ptr()
        arg.flags = (L.MPPI_AUTO_RESET if auto_reset else 0) | (L.MPPI_KEEP_MEAN if keep_mean else 0)
        arg.reserved = 0
        self._torch_call(self._lib.mt_mppi, C.byref(arg), commits=bool(commit and T))
        return out

    # ---- inverse kinematics: the Jacobian of the pickup frame and a damped-least-squares solver ----------------------------
    def _ik_rows(self, t, name, rows):
        """`rows` rows of per-env floats as the library reads them -> (float32 device tensor of shape (rows, N), ld).  A CUDA
        float32 (rows, N) tensor with unit env stride and a row pitch >= N -- a [..., :N] view of a wider buffer included --
        goes in zero-copy; an (N, rows) tensor, a numpy array or nested lists of either shape become a contiguous copy."""
        import torch
        dev = torch.device("cuda", self.device)
        n = self.n_envs
        if _is_torch_tensor(t):
            t = t.detach()
            if t.dim() == 2 and tuple(t.shape) == (rows, n) and t.dtype == torch.float32 and t.device == dev:
                _, ld = self._log_rows(t, name, None, torch.float32)
                return t, ld
        else:
            t = torch.from_numpy(np.array(t, dtype=np.float32))
        if t.dim() != 2 or tuple(t.shape) not in ((rows, n), (n, rows)):
            raise ValueError(f"{name} must be ({rows}, {n}) or ({n}, {rows}), got {tuple(t.shape)}")
        if tuple(t.shape) != (rows, n):
            t = t.t()
        return t.to(device=dev, dtype=torch.float32).contiguous(), n

    def _ik_vector(self, t, name, dtype):
        import torch
        dev = torch.device("cuda", self.device)
        if (not _is_torch_tensor(t) or t.dtype != dtype or t.device != dev or tuple(t.shape) != (self.n_envs,)
                or (self.n_envs > 1 and t.stride(0) != 1)):
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape ({self.n_envs},) on {dev}")
        return t

    def jacobian(self, angles=None, out=None, position=False):
        """The position Jacobian of the pickup frame (mt_jacobian) as a (3, D, N) float32 device tensor: [a, j, i] =
        d p_a / d q_j of env i per DEGREE -- column j is z_j x (p - o_j) * pi / 180, exactly 0 for a joint behind the
        driven frame (ee_frame).  angles: (D, N) degrees (read in place when a float32 device tensor, [..., :N] views
        included) or (N, D); None = the resident pose.  out: a (3, D, N) tensor to write into whose memory runs (D, 3, ld),
        e.g. buf.view(D, 3, ld)[..., :N].permute(1, 0, 2).  position=True returns (jacobian, p) with p (3, N), the driven
        point.  One launch; stream behaviour as rollout_actions; nothing resident is written."""
        import torch
        dev = torch.device("cuda", self.device)
        n, d = self.n_envs, self.dof
        ang, ang_ld = (None, n) if angles is None else self._ik_rows(angles, "angles", d)
        if out is None:
            out = torch.empty((d, 3, n), dtype=torch.float32, device=dev).permute(1, 0, 2)
        if not _is_torch_tensor(out) or out.dim() != 3 or tuple(out.shape) != (3, d, n):
            raise ValueError(f"out must be a float32 tensor of shape (3, {d}, {n}) on {dev}")
        _, jac_ld = self._log_rows(out.permute(1, 0, 2), "out", 3, torch.float32)
        pos = torch.empty((3, n), dtype=torch.float32, device=dev) if position else None
        self._torch_call(self._lib.mt_jacobian, ang.data_ptr() if ang is not None else None, ang_ld, out.data_ptr(), jac_ld,
                         pos.data_ptr() if position else None, n, commits=False)
        del ang
        return (out, pos) if position else out

    def ik(self, targets=None, start=None, *, iters=16, damping=2.0, max_step=30.0, tol=0.0, wrap=True, stage=False,
           residual=True, steps=False, index=None, angles=True):
        """Which joint angles put the pickup frame on that point?  `iters` damped-least-squares iterations per env in ONE
        launch (mt_ik): e = x - p(q); dq = degrees(J^T (J J^T + damping^2 I)^-1 e), scaled so that no joint moves more than
        `max_step` degrees per iteration; q += dq.  targets: (3, N) or (N, 3) points; None = each env's nearest alive target
        (squared Euclidean distance from the pickup frame at the start pose, lowest index on a tie).  start: (D, N) or
        (N, D) degrees; None = the resident pose.  Float32 device tensors of shape (rows, N) are read in place, [..., :N]
        views of wider buffers included.  tol > 0: an env whose box residual max |e_a| is <= tol before an iteration stops
        there -- bit for bit the angles of a call with that many iterations.  wrap=True maps the angles into [-180, 180)
        (action_sample's domain); wrap=False keeps them continuous from the start pose, the short route for step().
        stage=True also writes the angles to the action buffer: ik(stage=True) then step() is a scripted reach controller.
        Returns a dict of device tensors: `angles` (D, N) float32, `residual` (N,) float32 -- the box residual at the
        angles returned -- `steps` (N,) int32 and, in nearest mode (index=None means "then"), `index` (N,) int32, -1 for an
        env without an alive target (held at its start pose, residual 0).  A non-finite target or an unusable start angle
        holds that env too, with residual NaN.  Each of angles / residual / steps / index may be False, True or a tensor
        to write into (`angles`: a [..., :N] view of a wider buffer included).  Stream behaviour as rollout_actions."""
        import torch
        dev = torch.device("cuda", self.device)
        n, d = self.n_envs, self.dof
        iters = int(iters)
        if not 1 <= iters <= L.IK_MAX_ITERS:
            raise ValueError(f"iters must be 1..{L.IK_MAX_ITERS}, got {iters}")
        damping, max_step, tol = (float(np.float32(v)) for v in (damping, max_step, tol))
        if not (np.isfinite(damping) and damping > 0):
            raise ValueError(f"damping must be finite and > 0, got {damping!r}")
        if not (np.isfinite(max_step) and max_step > 0):
            raise ValueError(f"max_step must be finite and > 0, got {max_step!r}")
        if not (np.isfinite(tol) and tol >= 0):
            raise ValueError(f"tol must be finite and >= 0, got {tol!r}")
        nearest = targets is None
        index_given = _is_torch_tensor(index)
        if not nearest and (index_given or index):
            raise ValueError("index is the nearest-target mode's output: targets must be None")
        index = nearest if index is None else index
        arg = L.MtIk()
        arg.struct_size = C.sizeof(L.MtIk)
        arg.iters, arg.damping, arg.max_step_deg, arg.tol = iters, damping, max_step, tol
        arg.flags = (L.IK_STAGE if stage else 0) | (L.IK_WRAP if wrap else 0)
        tgt, sta = None, None
        if not nearest:
            tgt, arg.target_ld = self._ik_rows(targets, "targets", 3)
            arg.target = tgt.data_ptr()
        if start is not None:
            sta, arg.start_ld = self._ik_rows(start, "start", d)
            arg.start = sta.data_ptr()
        res = {}
        if _is_torch_tensor(angles) or angles:
            res["angles"] = angles if _is_torch_tensor(angles) else torch.empty((d, n), dtype=torch.float32, device=dev)
            rows, arg.angles_ld = self._log_rows(res["angles"], "angles", None, torch.float32)
            if rows != d:
                raise ValueError(f"angles must have D = {d} rows")
            arg.angles_out = res["angles"].data_ptr()
        for name, want, field, dtype in (("residual", residual, "residual_out", torch.float32),
                                         ("steps", steps, "iters_out", torch.int32), ("index", index, "index_out", torch.int32)):
            if _is_torch_tensor(want) or want:
                res[name] = self._ik_vector(want, name, dtype) if _is_torch_tensor(want) else torch.empty(n, dtype=dtype, device=dev)
                setattr(arg, field, res[name].data_ptr())
        if not res and not stage:
            raise ValueError("nothing to compute: no output asked for and stage=False")
        arg.reserved = 0
        self._torch_call(self._lib.mt_ik, C.byref(arg), commits=bool(stage))
        del tgt, sta
        return res

    def observe(self):
        """Environment.get_observations (manytor.py:141-153); result in field OBS."""
        self._call(self._lib.mt_observe)
        self.version += 1

    def check_done(self):
        """Environment.is_done (manytor.py:155-173); result in field DONE."""
        self._call(self._lib.mt_check_done)
        self.version += 1

    # ---- state access -------------------------------------------------------------------------
    def _shape_dtype(self, field):
        n, d, k = self.n_envs, self.dof, self.obj_number
        return {
            L.F_ACTIONS: ((n, d), np.float32), L.F_GOALS: ((n, d), np.float32), L.F_POINTS: ((n, k, 3), np.float32),
            L.F_ALIVE: ((n, k), np.uint8), L.F_OBS: ((n, 3 * k), np.float32), L.F_REWARD: ((n,), np.int32),
            L.F_DONE: ((n,), np.uint8), L.F_DONE_BITS: (((n + 63) // 64,), np.uint64), L.F_EE: ((n, 3), np.float32),
            L.F_TOTAL_REWARD: ((n,), np.float32), L.F_JOINTS: ((n, d, 3), np.float32),
            L.F_EPISODES: ((n,), np.uint32), L.F_LAST_RETURN: ((n,), np.float32),
            L.F_RETURN_RING: ((n, self.return_ring_slots), np.float32), L.F_TRACE: ((n, self.substeps, 3), np.float32),
            L.F_ZMIN: ((n,), np.float32),
        }[field]

    def get(self, field) -> np.ndarray:
        """Host copy of a field in the reference's shape (leading env axis)."""
        shape, dt = self._shape_dtype(field)
        out = np.empty(shape, dtype=dt)
        self._call(self._lib.mt_get, field, out.ctypes.data_as(C.c_void_p), C.c_int64(out.nbytes), 0)
        return out

    def set(self, field, value):
        shape, dt = self._shape_dtype(field)
        v = np.ascontiguousarray(np.asarray(value).astype(dt).reshape(shape))
        self._call(self._lib.mt_set, field, v.ctypes.data_as(C.c_void_p), C.c_int64(v.nbytes))
        self.version += 1

    def device_ptr(self, field):
        ptr, rows, ld, dt = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int()
        self._call(self._lib.mt_device_ptr, field, C.byref(ptr), C.byref(rows), C.byref(ld), C.byref(dt))
        return ptr.value, rows.value, ld.value, dt.value

    @property
    def ld(self) -> int:
        return self.device_ptr(L.F_REWARD)[2]      # any field: the row stride is the handle's (not F_GOALS: see mt_device_ptr)

    def device_tensor(self, field):
        """Zero-copy torch view of the resident SoA buffer: shape (rows, N) (or (N,) for single-row fields,
        (ceil(N/64),) for DONE_BITS).  `.T` gives the reference's (N, rows) orientation."""
        import torch
        ptr, rows, ld, dt = self.device_ptr(field)
        es = np.dtype(_NP_OF_DT[dt]).itemsize
        n = (self.n_envs + 63) // 64 if field == L.F_DONE_BITS else self.n_envs
        if dt in (L.DT_U32, L.DT_U64):      # torch has limited unsigned support: expose as same-width signed
            typestr = "<i4" if dt == L.DT_U32 else "<i8"
        else:
            typestr = _TYPESTR[dt]
        shape, strides = ((n,), (es,)) if rows == 1 else ((rows, n), (ld * es, es))
        holder = _CudaArrayHolder(ptr, shape, strides, typestr, self)
        t = torch.as_tensor(holder, device=f"cuda:{self.device}")
        t._manytor_owner = holder
        return t

    # ---- checkpoint / resume (the reference keeps its state in attributes, manytor.py:131-139) --------
    def get_state(self) -> dict:
        """Host copy of everything later calls depend on: joint angles, targets, alive flags, returns, done flags,
        per-env episode counters, last returns, the return ring and the episode base (+ the step outputs a caller may
        want to keep).  set_state() of this dict on an engine of the same shape resumes bit-identically: step(),
        reset_done(), finished() and return_ring() all continue as in the original run."""
        st = {"goals": self.goals(), "points": self.points(), "alives": self.alives(), "total_reward": self.total_reward(),
              "obs": self.obs(), "reward": self.reward(), "done": self.get(L.F_DONE), "ee": self.ee(),
              "episodes": self.episodes(), "last_return": self.last_return(), "episode0": int(self.episode0)}
        if self.return_ring_slots:
            st["return_ring"] = self.return_ring()
        return st

    def set_state(self, state: dict):
        """Restore from get_state(): goals / points / alives / total_reward, and -- when present -- the raw done bytes
        (incl. 2 = finished and already re-armed), episode counters, last returns, return ring and episode base."""
        if not getattr(self, "_armed", False):
            # a fresh handle has to be reset once before it can step; the values are overwritten right below
            self.reset(np.asarray(state["points"], dtype=np.float32))
        self.set(L.F_POINTS, state["points"])
        self.set(L.F_GOALS, state["goals"])
        self.set(L.F_ALIVE, np.asarray(state["alives"]).astype(np.uint8))
        self.set(L.F_TOTAL_REWARD, state["total_reward"])
        for key, field in (("done", L.F_DONE), ("episodes", L.F_EPISODES), ("last_return", L.F_LAST_RETURN)):
            if key in state:
                self.set(field, state[key])
        if "return_ring" in state and self.return_ring_slots:
            self.set(L.F_RETURN_RING, state["return_ring"])
        if "episode0" in state:
            self.episode0 = int(state["episode0"])
            self._call(self._lib.mt_set_episode_base, C.c_uint32(self.episode0))

    # convenience getters in the reference's vocabulary
    def goals(self):
        return self.get(L.F_GOALS)

    def points(self):
        return self.get(L.F_POINTS)

    def alives(self):
        return self.get(L.F_ALIVE).astype(bool)

    def obs(self):
        return self.get(L.F_OBS)

    def reward(self):
        return self.get(L.F_REWARD)

    def done(self):
        return self.get(L.F_DONE).astype(bool)

    def ground_hit(self):
        """(N,) bool: the arm touched the ground at one of the sub-step poses of the last step (manytor.py:191-192).  The
        reference folds this into reward == -1 (:211-212) and does NOT end the episode on it;
        `terminate_on_ground=True` opts into ending it."""
        return self.get(L.F_REWARD) == -1

    def done_bits(self):
        return self.get(L.F_DONE_BITS)

    def ee(self):
        return self.get(L.F_EE)

    def total_reward(self):
        return self.get(L.F_TOTAL_REWARD)

    def joints_coordinates(self):
        return self.get(L.F_JOINTS)

    def episodes(self):
        return self.get(L.F_EPISODES)

    def last_return(self):
        return self.get(L.F_LAST_RETURN)

    def actions(self):
        return self.get(L.F_ACTIONS)

    def return_ring(self):
        """(N, R): slot c % R holds the return of the c-th episode the env finished since the last full reset."""
        return self.get(L.F_RETURN_RING)

    def finished(self):
        """(N,) number of episodes each env has finished (re-armed by reset_done / auto_reset) since the last full reset."""
        return (self.episodes() - np.uint32(self.episode0)).astype(np.int64)

    def zmin(self):
        """(N,) signed minimum z of the observation / pickup frames over all sub-step poses of the last step: the value
        the kernel's ground test compared with 0 (needs debug_zmin=True; manytor.py:191-192)."""
        return self.get(L.F_ZMIN)

    def trace(self):
        """(N, S, 3): end effector at each sub-step pose of the last step (needs trace=True; manytor.py:190)."""
        return self.get(L.F_TRACE)

    # ---- multi-GPU: the return gather -------------------------------------------------
    def comm_init(self, unique_id: bytes, rank: int, world_size: int):
        """Join the RCCL communicator named by `unique_id` (128 bytes from comm_unique_id() on rank 0).  Collective."""
        if len(unique_id) != L.MT_UNIQUE_ID_BYTES:
            raise ValueError("unique_id must be 128 bytes")
        buf = C.create_string_buffer(bytes(unique_id), L.MT_UNIQUE_ID_BYTES)
        self._call(self._lib.mt_comm_init, C.cast(buf, C.c_void_p), int(rank), int(world_size))

    def comm_destroy(self):
        self._call(self._lib.mt_comm_destroy)

    def total_envs(self) -> int:
        t = C.c_int64(0)
        self._call(self._lib.mt_comm_total_envs, C.byref(t))
        return int(t.value)

    def return_stats(self, field=None, row=0) -> dict:
        """{sum, min, max, mean, count, done} of a return row over ALL ranks (mt_reduce_returns): reduced on the device,
        five numbers per rank exchanged -- what a learner logs per episode without moving the row.  Synchronous;
        collective when a communicator is attached."""
        st = L.MtReturnStats()
        self._call(self._lib.mt_reduce_returns, int(L.F_TOTAL_REWARD if field is None else field), int(row), C.byref(st))
        return {"sum": st.sum, "min": st.min, "max": st.max, "mean": st.sum / max(1, st.count), "count": int(st.count),
                "done": int(st.done)}

    def _gather_out(self, out):
        import torch
        n_total = self.total_envs()
        if out is None:
            out = torch.empty(n_total, dtype=torch.float32, device=f"cuda:{self.device}")
        if out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or out.numel() != n_total:
            raise ValueError(f"out must be a contiguous float32 device tensor of {n_total} elements")
        return out, n_total

    def gather_begin(self, out=None, field=None, row=0, snapshot=True):
        """Start the all-gather of one return row on the engine's side stream and return at once: steps and resets queued
        next overlap with the exchange.  `out` is complete after gather_wait(host=True) or sync().  By default the row is
        snapshotted on the main stream first (so a reset queued next may overwrite it); `snapshot=False` lets the exchange
        read the row in place -- for MT_F_LAST_RETURN right after the reset that ended the episode (that row is written by
        resets only, and the library orders its later resets behind the exchange)."""
        field = L.F_TOTAL_REWARD if field is None else field
        out, n_total = self._gather_out(out)
        fn = self._lib.mt_gather_returns_begin if snapshot else self._lib.mt_gather_returns_begin_inplace
        self._call(fn, int(field), int(row), C.c_void_p(out.data_ptr()), C.c_int64(n_total))
        return out

    def gather_wait(self, host=False):
        """Order the engine's stream behind the last begun gather; host=True also blocks until its result is complete
        and returns the device milliseconds the exchange took."""
        ms = C.c_float(0)
        self._call(self._lib.mt_gather_returns_wait, 1 if host else 0, C.byref(ms))
        return ms.value if host else None

    def gather_returns(self, out=None, field=None, row=0):
        """All-gather one return row of every rank into `out`: a float32 device tensor of total_envs() elements (made
        if None), global env order.  RCCL straight from the arena on the engine's stream; a device copy on one GPU.
        Asynchronous: the result is ordered on the engine's stream (sync() or use_torch_stream() before reading)."""
        field = L.F_TOTAL_REWARD if field is None else field
        out, n_total = self._gather_out(out)
        self._call(self._lib.mt_gather_returns, int(field), int(row), C.c_void_p(out.data_ptr()), C.c_int64(n_total))
        return out


def comm_unique_id() -> bytes:
    """128 bytes naming a new RCCL communicator (call on rank 0, ship to the other ranks, then comm_init everywhere)."""
    lib = L.load()
    buf = C.create_string_buffer(L.MT_UNIQUE_ID_BYTES)
    L.check(lib.mt_comm_unique_id(C.cast(buf, C.c_void_p)))
    return buf.raw


# ---- stateless helpers = module functions of the reference (manytor.py:17-53) -------------------
def stream_probe(n_envs, dof=4, obj_number=7, reps=50, device=0):
    """(us per pass, bytes per pass) of the streaming yardstick: the memory operations of one step_random over n_envs
    envs -- same rows, same stores, same addressing -- without its arithmetic (mt_stream_probe)."""
    us, nbytes = C.c_float(0), C.c_int64(0)
    L.check(L.load().mt_stream_probe(int(device), int(dof), int(obj_number), C.c_int64(int(n_envs)), int(reps), C.byref(us),
                                     C.byref(nbytes)))
    return us.value, nbytes.value


def fk_batch(mode, angles, dh_table=REF_DH_TABLE, radians=False, device=0) -> np.ndarray:
    lib = L.load()
    table = np.ascontiguousarray(np.asarray(dh_table, dtype=np.float32))
    dof = table.shape[0]
    a = np.ascontiguousarray(np.asarray(angles, dtype=np.float32).reshape(-1, dof))
    out = np.empty((a.shape[0], 4, 4), dtype=np.float32)
    L.check(lib.mt_fk_batch(device, table.ctypes.data_as(C.c_void_p), dof, int(mode), a.ctypes.data_as(C.c_void_p),
                            1 if radians else 0, C.c_int64(a.shape[0]), out.ctypes.data_as(C.c_void_p)))
    return out


def route_trace(prev, action, dh_table=REF_DH_TABLE, substeps=25, device=0) -> np.ndarray:
    """joints_coordinates at every sub-step pose of the routes prev[i] -> action[i] (manytor.py:182-190):
    (n, dof) degrees in, (n, substeps, dof, 3) out."""
    lib = L.load()
    table = np.ascontiguousarray(np.asarray(dh_table, dtype=np.float32))
    dof = table.shape[0]
    p = np.ascontiguousarray(np.asarray(prev, dtype=np.float32).reshape(-1, dof))
    a = np.ascontiguousarray(np.asarray(action, dtype=np.float32).reshape(-1, dof))
    if p.shape != a.shape:
        raise ValueError("prev and action must have the same shape")
    out = np.empty((p.shape[0], int(substeps), dof, 3), dtype=np.float32)
    L.check(lib.mt_route_trace(device, table.ctypes.data_as(C.c_void_p), dof, int(substeps), p.ctypes.data_as(C.c_void_p),
                               a.ctypes.data_as(C.c_void_p), C.c_int64(p.shape[0]), out.ctypes.data_as(C.c_void_p)))
    return out


def r_theta_batch(v1, v2, device=0) -> np.ndarray:
    lib = L.load()
    a = np.ascontiguousarray(np.asarray(v1, dtype=np.float32).reshape(-1, 3))
    b = np.ascontiguousarray(np.asarray(v2, dtype=np.float32).reshape(-1, 3))
    out = np.empty((a.shape[0], 2), dtype=np.float32)
    L.check(lib.mt_r_theta_batch(device, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                 C.c_int64(a.shape[0]), out.ctypes.data_as(C.c_void_p)))
    return out
