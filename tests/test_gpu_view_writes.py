"""Writes through zero-copy device views on a caller's stream, held to the fp64 oracle.

The documented policy loop (examples/policy_loop.py) puts the handle on torch's stream (use_torch_stream),
takes the views of the resident rows ONCE (device_tensor) and never synchronises with the host: a torch op queued between
two library calls must be seen by the second one (include/manytor_hip.h: on a caller's stream, stream order is the whole
contract).  The library keeps host-side knowledge about device state that such a write can contradict -- every angle is a
whole degree, the target codes match the floats, the gather's snapshot row already holds the returns, a full reset is still
pending -- and these tests write every writable row through its view in front of every consumer, at
every form mt_rollout takes (five steps per launch over 4 / 2 lanes, a replayed HIP graph, two chains joined per call, the
default two chains of the large batches).

How a case runs: the oracle (oracle/c_oracle.py, driven with the action / target streams of oracle/philox_ref.py) plays the
whole script on the host first and records it as a program; every edit is an fp32 array computed there (a relocated target
needs the oracle's end effector) and uploaded; one torch.cuda.synchronize(); then the program is replayed on the GPU.  Between
the library call in front of an edit and the call that consumes it the host never waits.  Checkpoints come after the
consumer: they read with the host getters, compare, and put the envs whose oracle margin to a threshold (z = 0, |delta| =
tol) was below GUARD back onto the oracle's state with eng.set, since fp32 and fp64 may decide those differently.

The own-stream control runs the same programs on the handle's private stream by the header's rule for that mode: eng.sync()
before a foreign write, torch.cuda.synchronize() after it.

Tolerances are parity_util's: POS_TOL for end effector and z-minimum, assert_obs_close for observations, everything else
exact outside the guard band.  One exception to "every env" for the z-minimum, stated here because it is a property of the
comparison and not of the kernels: inside mt_rollout_fused(auto_reset) an env whose pickup decision sat in the guard band
may have been re-armed (pose zeroed) on one side only, and the NEXT step's route then starts from different poses; such
envs are left out of that call's z-minimum (their end effector, which depends on the action alone, is still compared)."""
import copy

import numpy as np
import pytest

import staged_populations as sp
from parity_util import GUARD, POS_TOL, assert_obs_close

pytestmark = pytest.mark.gpu

SEED = 0x51DE
RING = 4
BONUSES = np.array([-2.5, -0.5, 0.5, 3.0], dtype=np.float32)     # every sum of these and of +-1 rewards is exact in fp32


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


# n, K, table, MT_* overrides, and what eng.dispatch() must say about mt_rollout: the smallest sizes that reach each form
REGIMES = {
    "k5_lanes4": dict(n=3001, k=7, table="ref", env={},
                      rollout=dict(form="multi_step", steps_per_launch=5, lanes_per_env=4, chains=1, absorbs_reset=True)),
    "k5_lanes2": dict(n=70001, k=3, table="dh7", env={},
                      rollout=dict(form="multi_step", steps_per_launch=5, lanes_per_env=2, chains=1, absorbs_reset=True)),
    "graph": dict(n=9001, k=7, table="ref", env={"MT_ROLLOUT_K": "1"},
                  rollout=dict(form="graph_replay", steps_per_launch=1, graph=True, chains=1)),
    "two_chains": dict(n=9001, k=3, table="rt5", env={"MT_ROLLOUT_K": "1", "MT_GRAPH": "0", "MT_CHAINS": "2"},
                       rollout=dict(form="chained_steps", steps_per_launch=1, graph=False, chains=2)),
    "large": dict(n=300007, k=7, table="ref", env={},
                  rollout=dict(form="chained_steps", steps_per_launch=1, graph=False, chains=2)),
}


def _table(m, name):
    if name == "rt5":
        return sp.fractional_offset_table()
    return {"ref": (m.REF_DH_TABLE, 51.3), "dh7": (m.DH7_TABLE, 92.6)}[name]


def _make(m, monkeypatch, regime, on_torch_stream):
    """The engine of a regime (dispatch asserted), reset, and its oracle mirror."""
    cfg = REGIMES[regime]
    for key, val in cfg["env"].items():
        monkeypatch.setenv(key, val)
    table, radius = _table(m, cfg["table"])
    eng = m.StepEngine(cfg["n"], cfg["k"], dh_table=table, radius=radius, debug_zmin=True, return_ring=RING)
    d = eng.dispatch()
    for key, val in cfg["rollout"].items():
        assert d["rollout"][key] == val, (regime, key, d["rollout"])
    for key, val in cfg["env"].items():
        assert f"{key}={val}" in d["overrides"], d["overrides"]
    if on_torch_stream:
        eng.use_torch_stream()
    eng.reset_random(SEED, 0)
    return eng, Mirror(cfg["n"], cfg["k"], np.asarray(table, dtype=np.float64), radius)


class Mirror:
    """The oracle side of a script.  Every method applies one library call or one torch write to the fp64 state and appends
    the same operation to `program`, which replay() later runs on the GPU."""

    def __init__(self, n, k, table, radius):
        from oracle import c_oracle
        from oracle import philox_ref as px
        self.px = px
        self.n, self.k, self.dof, self.table, self.radius = n, k, table.shape[0], table, radius
        self.ora = c_oracle.COracle(n, k, table=table, radius=radius)
        self.fk = c_oracle.COracle(n, 1, table=table, substeps=2)      # forward kinematics alone (ee_of)
        self.ids = np.arange(n, dtype=np.uint64)
        self.rng = np.random.RandomState(n + 31 * k)
        self.program = []
        self.uploads = []                                   # fp32 host arrays of the edits, uploaded before the replay
        self.episode0 = 0
        self.episodes = np.zeros(n, dtype=np.int64)
        self.last_return = np.zeros(n)
        self.ring = np.zeros((n, RING))
        self.ring_known = np.zeros((n, RING), dtype=bool)   # slots written since the mirror started
        self.done = np.zeros(n, dtype=np.uint8)             # the raw byte: 0, 1 = finished, 2 = finished and re-armed
        self.reward = np.zeros(n, dtype=np.int64)
        self.last = None                                    # outputs of the last step
        self.risky = np.zeros(n, dtype=bool)                # envs that touched the guard band since the last checkpoint
        self.zmin_free = np.zeros(n, dtype=bool)            # ... in a re-arming call, ahead of its last step (module docstring)
        self.stats = dict(env_steps=0, guarded=0, picked=0, grounded=0, airborne=0, dones=0)
        self.tapes = []                                     # fp32 (T, n, D) action tapes, uploaded before the replay
        self.tape_calls = []                                # tape calls since the last checkpoint: their expected logs
        self.tape_pairs = []                                # ... and pairs of them whose logs must be the same bits
        self.bad_actions = 0                                # (env, step) pairs a committing tape call held
        self._full_reset(0)

    # ---- state transitions -------------------------------------------------------------------
    def _full_reset(self, episode):
        o = self.ora
        self.last_return = o.total_reward.copy()
        o.reset(self.px.sample_targets(SEED, self.ids, episode, self.k, self.radius).astype(np.float64))
        self.episodes[:] = episode
        self.episode0 = episode
        self.done[:] = 0
        self.reward[:] = 0

    def _rearm(self, idx):
        o = self.ora
        if idx.size == 0:
            return
        slot = (self.episodes[idx] - self.episode0) % RING
        self.ring[idx, slot] = o.total_reward[idx]
        self.ring_known[idx, slot] = True
        self.last_return[idx] = o.total_reward[idx]
        self.episodes[idx] += 1
        o.goals[idx] = 0.0
        o.total_reward[idx] = 0.0
        o.alive_u8[idx] = 1
        o.points[idx] = self.px.sample_targets(SEED, self.ids[idx], self.episodes[idx], self.k, self.radius).astype(np.float64)

    def _step(self, actions, rearm=False, last_of_call=True):
        o = self.ora
        pre_alive = o.alives.copy()
        obs, rew, done = o.step(actions)
        pm = np.where(pre_alive, o.pickup_margin, np.inf).min(axis=1)
        risky = (o.ground_margin < GUARD) | (pm < GUARD)
        self.risky |= risky
        if rearm and not last_of_call:
            self.zmin_free |= self.risky
        s = self.stats
        s["env_steps"] += self.n
        s["guarded"] += int(risky.sum())
        s["picked"] += int(pre_alive.sum() - o.alives.sum())
        s["grounded"] += int((rew == -1).sum())
        s["airborne"] += int((rew != -1).sum())
        s["dones"] += int(done.sum())
        self.reward = rew
        self.done = done.astype(np.uint8)
        if last_of_call:
            self.last = dict(obs=obs, elbow=o.joints_coordinates[:, -2].copy(), ee=o.joints_coordinates[:, -1].copy(),
                             points=o.points.copy(), pre_alive=pre_alive, zmin=o.zmin.copy())
        if rearm:
            self._rearm(np.flatnonzero(done))
            self.done[done] = 2

    def _actions(self, t):
        return self.px.sample_actions(SEED, self.ids, t, self.dof).astype(np.float64)

    def joints_of(self, pose):
        """joints_coordinates (fp64) of a pose: the oracle's own chain, at the end of a step that starts and ends there."""
        self.fk.goals[:] = pose
        self.fk.step(pose)
        return self.fk.joints_coordinates.copy()

    def ee_of(self, pose):
        """End effector of a pose: where a target has to go to be picked by the step that ends there."""
        return self.joints_of(pose)[:, -1]

    # ---- library calls -----------------------------------------------------------------------
    def step_random(self, t):
        self._step(self._actions(t))
        self.program.append(("call", lambda e: e.step_random(SEED, t)))

    def rollout(self, T, t0):
        for t in range(t0, t0 + T):
            self._step(self._actions(t), last_of_call=t == t0 + T - 1)
        self.program.append(("call", lambda e: e.rollout(T, SEED, t0)))

    def rollout_fused(self, T, t0, auto_reset=False):
        for t in range(t0, t0 + T):
            self._step(self._actions(t), rearm=auto_reset, last_of_call=t == t0 + T - 1)
        self.program.append(("call", lambda e: e.rollout_fused(T, SEED, t0, auto_reset=auto_reset)))

    def step_staged(self, actions32):
        """eng.step() on the actions a torch write left in MT_F_ACTIONS."""
        self.edit("F_ACTIONS", actions32.T)
        self._step(actions32.astype(np.float64))
        self.program.append(("call", lambda e: e.step()))

    def observe(self):
        o = self.ora
        o.joints_coordinates = self.joints_of(o.goals)
        pre_alive = o.alives.copy()
        obs = o.get_observations()                           # also zeroes the coordinates of dead targets
        self.last = dict(obs=obs, elbow=o.joints_coordinates[:, -2].copy(), points=o.points.copy(), pre_alive=pre_alive)
        self.program.append(("call", lambda e: e.observe()))

    def check_done(self):
        o = self.ora
        ee = self.ee_of(o.goals)
        delta = np.abs(ee[:, None, :] - o.points)
        pre_alive = o.alives.copy()
        hit = np.all(delta <= o.pickup_tol, axis=-1) & pre_alive
        margin = np.where(pre_alive, np.abs(delta - o.pickup_tol).min(axis=-1), np.inf).min(axis=1)
        self.risky |= margin < GUARD
        self.stats["picked"] += int(hit.sum())
        o.alive_u8[hit] = 0
        self.done = (~o.alives.any(axis=1)).astype(np.uint8)
        self.program.append(("call", lambda e: e.check_done()))

    def reset_random(self, episode):
        self._full_reset(episode)
        self.program.append(("call", lambda e: e.reset_random(SEED, episode)))

    def reset_done(self):
        self._rearm(np.flatnonzero(self.done == 1))
        self.done[:] = 0
        self.program.append(("call", lambda e: e.reset_done(SEED)))

    def take_views(self, *fields):
        self.program.append(("views", fields))

    # ---- mt_rollout_tape ---------------------------------------------------------------------------
    _MIRRORED = ("episode0", "episodes", "last_return", "ring", "ring_known", "done", "reward", "last", "risky", "zmin_free",
                 "stats", "bad_actions")
    _ORACLE = ("goals", "points", "alive_u8", "total_reward", "joints_coordinates", "ground_margin", "pickup_margin",
               "ground_hit", "zmin")

    def rollout_actions(self, tape32, auto_reset=False, dry_run=False, compare_resident=True):
        """eng.rollout_actions(tape, log=True, returns=True) on an fp32 (T, n, D) tape: T oracle steps, an unusable angle
        (kernels.h: unusable_angle) holds the pose, finished envs are re-armed as _rearm does, only the last row leaves
        outputs.  The logs and `returns` are compared at the next checkpoint, for the envs outside the guard band.  A dry
        run plays the same steps for its logs and puts the oracle back; on the GPU everything resident is compared bit for bit
        with a host snapshot taken in front of the call (compare_resident=False: no snapshot, hence no host wait in front of
        the call).  Returns the call's record (for expect_same_logs)."""
        tape32 = np.ascontiguousarray(tape32, dtype=np.float32)
        assert tape32.shape[1:] == (self.n, self.dof) and not (auto_reset and dry_run)
        T = tape32.shape[0]
        keep = None
        if dry_run:
            keep = ({f: copy.deepcopy(getattr(self, f)) for f in self._MIRRORED},
                    {f: getattr(self.ora, f).copy() for f in self._ORACLE})
        rew, done, held = [], [], 0
        for t in range(T):
            bad = (~np.isfinite(tape32[t]) | (np.abs(tape32[t]) > sp.LIMIT)).any(axis=1)
            held += int(bad.sum())
            self._step(np.where(bad[:, None], self.ora.goals, tape32[t].astype(np.float64)), rearm=auto_reset,
                       last_of_call=t == T - 1)
            rew.append(self.reward.copy())
            done.append(self.done != 0)
        call = dict(slot=len(self.tapes), T=T, auto_reset=auto_reset, dry=dry_run, compare_resident=compare_resident,
                    reward=np.stack(rew).astype(np.int8), done=np.stack(done).astype(np.uint8),
                    returns=np.stack(rew).sum(axis=0).astype(np.float32), risky=self.risky.copy(), res=None)
        if dry_run:
            for f, v in keep[0].items():
                setattr(self, f, v)
            for f, v in keep[1].items():
                setattr(self.ora, f, v)
        else:
            self.bad_actions += held
        self.tapes.append(tape32)
        self.tape_calls.append(call)
        self.program.append(("tape", call))
        return call

    def expect_same_logs(self, a, b):
        """The logs and returns of two tape calls (a dry run and the committing call of the same rows): the same bits."""
        self.tape_pairs.append((a, b))

    def _return_row(self, field):
        return dict(F_TOTAL_REWARD=self.ora.total_reward, F_LAST_RETURN=self.last_return)[field].astype(np.float32)

    def gather_begin(self, key, field="F_TOTAL_REWARD", snapshot=True):
        """eng.gather_begin of a return row (snapshot=False: the exchange reads the row in place).  The buffer must hold the
        row as it is NOW; the envs that are in the guard band now are left out."""
        self.program.append(("gather_begin", key, field, snapshot, self._return_row(field), self.risky.copy()))

    def gather_end(self, key, stale=None, must_differ=0.1):
        """gather_wait(host) of gather_begin(key).  `stale` is what a wrong order would ship -- the row at another time, by
        default as it is now, behind the calls queued since gather_begin -- and has to differ from the expected row in at
        least `must_differ` of the envs, so that order is really what the comparison decides."""
        begin = next(op for op in reversed(self.program) if op[0] == "gather_begin" and op[1] == key)
        stale = self._return_row(begin[2]) if stale is None else np.asarray(stale, dtype=np.float32)
        assert (stale != begin[4]).mean() > must_differ, (stale != begin[4]).mean()
        self.program.append(("gather_end", key, stale))

    # ---- torch writes through the views --------------------------------------------------------
    def edit(self, field, rows32, rows=None):
        """view[:rows] = rows32 (an fp32 array in the view's (rows, n) orientation)."""
        slot = len(self.uploads)
        self.uploads.append(np.ascontiguousarray(rows32, dtype=np.float32))
        self.program.append(("edit", lambda v, up: (v[field] if rows is None else v[field][:rows]).copy_(up[slot])))

    def edit_goals(self, kind):
        n, d = self.n, self.dof
        if kind == "fractional":
            g = self.rng.uniform(-150.0, 150.0, size=(n, d)).astype(np.float32)
        elif kind == "turns":                                # whole turns out to +-32 400 degrees: the wide route
            g = sp.local_turns(int(self.rng.randint(1 << 30)), n, d)[0]
        elif kind == "whole":                                # back to whole degrees
            g = self.rng.randint(-180, 180, size=(n, d)).astype(np.float32)
        else:
            raise AssertionError(kind)
        self.ora.goals[:] = g.astype(np.float64)
        self.edit("F_GOALS", g.T)

    def edit_points_near(self, pose):
        """Targets 0 .. min(3, K) - 1 to the end effector of `pose` + uniform(-12, 12) per axis (tol 8: about 30 % are picked
        by the step that ends at `pose`; continuous offsets, so the threshold itself stays rare)."""
        mm = min(3, self.k)
        p = (self.ee_of(pose)[:, None, :] + self.rng.uniform(-12.0, 12.0, size=(self.n, mm, 3))).astype(np.float32)
        self.ora.points[:, :mm] = p.astype(np.float64)
        self.edit("F_POINTS", p.reshape(self.n, 3 * mm).T, rows=3 * mm)

    def edit_alive(self):
        """Clear bit K-1 of every third env (its coordinates stay: the next step has to zero them, manytor.py:148), then set
        all K bits of every fifth env (targets that were picked come back where the zeroing left them)."""
        k = self.k
        self.ora.alive_u8[::3, k - 1] = 0
        self.ora.alive_u8[::5, :] = 1
        self.program.append(("edit", lambda v, up: (v["F_ALIVE"][::3].bitwise_and_(~(1 << (k - 1))),
                                                    v["F_ALIVE"][::5].fill_((1 << k) - 1))))

    def edit_kill(self, stride):
        """Clear every alive bit of every stride-th env: done at its next step."""
        self.ora.alive_u8[::stride, :] = 0
        self.program.append(("edit", lambda v, up: v["F_ALIVE"][::stride].fill_(0)))

    def edit_bonus(self):
        """total_reward += a per-env bonus; returns what the row would hold WITHOUT it (the check that the edit matters)."""
        b = BONUSES[self.rng.randint(0, 4, size=self.n)]
        without = self.ora.total_reward.copy()
        self.ora.total_reward += b.astype(np.float64)
        slot = len(self.uploads)
        self.uploads.append(b)
        self.program.append(("edit", lambda v, up: v["F_TOTAL_REWARD"].add_(up[slot])))
        return without

    # ---- consumers with a result of their own ------------------------------------------------------
    def gather(self, how, without):
        """how: 'returns' (in line), 'begin' (side stream: gather_begin + gather_wait(host)) or 'stats' (return_stats)."""
        want = self.ora.total_reward.astype(np.float32)
        assert (want != without.astype(np.float32)).mean() > 0.9            # the bonus changed what must come out
        self.program.append(("gather", how, want, without.astype(np.float32), self.risky.copy()))

    # ---- checkpoints -----------------------------------------------------------------------------
    def check(self, what="step", label=""):
        o = self.ora
        if self.tape_calls:                                  # the logs of the tape calls since the last checkpoint come first
            self.program.append(("tape_logs", self.tape_calls, self.tape_pairs, self.risky.copy(), self.bad_actions, label))
            self.tape_calls, self.tape_pairs = [], []
        exp = dict(what=what, label=label, ok=~self.risky, zmin_ok=~self.zmin_free,
                   goals=o.goals.astype(np.float32), points=o.points.astype(np.float32), alive=o.alives.copy(),
                   total=o.total_reward.astype(np.float32), episodes=self.episodes.copy(),
                   last_return=self.last_return.astype(np.float32), ring=self.ring.astype(np.float32),
                   ring_known=self.ring_known.copy(), done=self.done.copy(), reward=self.reward.copy(),
                   last=self.last, episode0=self.episode0)
        self.program.append(("check", exp))
        self.risky = np.zeros(self.n, dtype=bool)
        self.zmin_free = np.zeros(self.n, dtype=bool)


def _checkpoint(m, eng, exp):
    L = m.lib
    eng.sync()
    ok, what, tag = exp["ok"], exp["what"], exp["label"]
    got = dict(goals=eng.goals(), points=eng.points(), alive=eng.alives(), total=eng.total_reward(),
               episodes=eng.episodes().astype(np.int64), last_return=eng.last_return(), ring=eng.return_ring(),
               done=eng.get(L.F_DONE))
    last = exp["last"]
    if what == "step":
        assert np.abs(eng.ee() - last["ee"]).max() <= POS_TOL, tag                      # every env, guard band or not
        zerr = np.abs(eng.zmin() - last["zmin"])[exp["zmin_ok"]]
        assert zerr.max() <= POS_TOL, (tag, zerr.max())
        np.testing.assert_array_equal(eng.reward()[ok], exp["reward"][ok], err_msg=tag)
    if what in ("step", "observe"):
        assert_obs_close(eng.obs()[ok], last["obs"][ok], last["elbow"][ok], last["points"][ok], last["pre_alive"][ok])
    if what != "reset":                                      # (a full reset clears the done bytes: nothing to compare)
        np.testing.assert_array_equal(got["done"][ok], exp["done"][ok], err_msg=tag)
        bits = eng.done_bits()
        unpacked = ((bits[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).ravel()[: ok.size]
        np.testing.assert_array_equal(unpacked, got["done"] != 0, err_msg=tag)
    for f in ("goals", "points", "alive", "total", "episodes", "last_return"):
        np.testing.assert_array_equal(got[f][ok], exp[f][ok], err_msg=f"{tag}: {f}")
    known = exp["ring_known"] & ok[:, None]
    np.testing.assert_array_equal(got["ring"][known], exp["ring"][known], err_msg=f"{tag}: ring")
    np.testing.assert_array_equal(eng.finished()[ok], (exp["episodes"] - exp["episode0"])[ok], err_msg=tag)
    idx = np.flatnonzero(~ok)
    if idx.size:                                             # guard-band envs: back onto the oracle's state
        for f, field in (("goals", L.F_GOALS), ("points", L.F_POINTS), ("total", L.F_TOTAL_REWARD), ("done", L.F_DONE),
                         ("episodes", L.F_EPISODES), ("last_return", L.F_LAST_RETURN), ("ring", L.F_RETURN_RING)):
            if not np.array_equal(got[f][idx], exp[f][idx]):
                got[f][idx] = exp[f][idx]
                eng.set(field, got[f])
        if not np.array_equal(got["alive"][idx], exp["alive"][idx]):
            got["alive"][idx] = exp["alive"][idx]
            eng.set(L.F_ALIVE, got["alive"].astype(np.uint8))


VIEW_FIELDS = ("F_GOALS", "F_POINTS", "F_ALIVE", "F_TOTAL_REWARD", "F_ACTIONS")


def replay(m, eng, mir, on_torch_stream):
    """Run the recorded program on the GPU.  On torch's stream nothing waits between a library call, the torch writes behind
    it and the call that consumes them; on the handle's own stream every write sits between eng.sync() and
    torch.cuda.synchronize(), as include/manytor_hip.h asks."""
    import torch
    dev = f"cuda:{eng.device}"
    up = [torch.from_numpy(a).to(dev) for a in mir.uploads]
    tapes = [torch.from_numpy(a).to(dev) for a in mir.tapes]
    views = {}
    gathers = {}
    torch.cuda.synchronize()
    gathered = 0
    for op in mir.program:
        kind = op[0]
        if kind == "views":
            for f in op[1]:
                views[f] = eng.device_tensor(getattr(m.lib, f))
        elif kind == "call":
            op[1](eng)
        elif kind == "edit":
            if not on_torch_stream:
                eng.sync()
            op[1](views, up)
            if not on_torch_stream:
                torch.cuda.synchronize()
        elif kind == "gather":
            _, how, want, without, risky = op
            ok = ~risky
            if how == "stats":
                st = eng.return_stats()
                assert not risky.any()                       # (scripted behind a checkpoint and a call that decides nothing)
                w64 = want.astype(np.float64)
                assert (st["sum"], st["min"], st["max"], st["count"]) == (w64.sum(), w64.min(), w64.max(), want.size), st
                assert st["sum"] != without.astype(np.float64).sum()
            else:
                if how == "begin":
                    buf = eng.gather_begin()
                    eng.gather_wait(host=True)
                else:
                    buf = eng.gather_returns()
                    eng.sync()
                    torch.cuda.synchronize()
                got = buf.cpu().numpy()
                stale = int((got[ok] == without[ok]).sum()) if not np.array_equal(got[ok], want[ok]) else 0
                np.testing.assert_array_equal(got[ok], want[ok], err_msg=f"gather {gathered} ({how}): {stale} of {int(ok.sum())} envs "
                                              "hold the returns from before the torch write")
            gathered += 1
        elif kind == "tape":
            _tape_call(m, eng, op[1], tapes)
        elif kind == "tape_logs":
            eng.sync()
            torch.cuda.synchronize()
            _check_tape_logs(eng, *op[1:])
        elif kind == "gather_begin":
            _, key, field, snapshot, want, risky = op
            gathers[key] = (eng.gather_begin(field=getattr(m.lib, field), snapshot=snapshot), want, ~risky)
        elif kind == "gather_end":
            buf, want, ok = gathers.pop(op[1])
            eng.gather_wait(host=True)
            got, stale = buf.cpu().numpy(), op[2]
            n_stale = int(((got == stale) & (got != want))[ok].sum())
            np.testing.assert_array_equal(got[ok], want[ok], err_msg=f"gather {op[1]}: {n_stale} of {int(ok.sum())} envs hold "
                                          "the row of another moment")
        elif kind == "check":
            _checkpoint(m, eng, op[1])
        else:
            raise AssertionError(kind)
    assert not mir.tape_calls and not gathers                # (a script ends with a checkpoint behind its last tape call)
    torch.cuda.synchronize()


RESIDENT = ("F_ACTIONS", "F_GOALS", "F_POINTS", "F_ALIVE", "F_TOTAL_REWARD", "F_EPISODES", "F_LAST_RETURN", "F_RETURN_RING",
            "F_OBS", "F_REWARD", "F_DONE", "F_DONE_BITS", "F_EE", "F_ZMIN")


def _tape_call(m, eng, call, tapes):
    """One tape call of the program.  The committing call waits for nothing beyond what eng.rollout_actions itself does."""
    before = None
    if call["dry"] and call["compare_resident"]:
        eng.sync()
        before = {f: eng.get(getattr(m.lib, f)) for f in RESIDENT}, eng.bad_action_count(), eng.version
    call["res"] = eng.rollout_actions(tapes[call["slot"]], auto_reset=call["auto_reset"], seed=SEED, log=True, returns=True,
                                      dry_run=call["dry"])
    if before is not None:
        eng.sync()
        for f, v in before[0].items():
            np.testing.assert_array_equal(eng.get(getattr(m.lib, f)), v, err_msg=f"{f} after a dry run")
        assert (eng.bad_action_count(), eng.version) == before[1:]


def _check_tape_logs(eng, calls, pairs, risky, bad_actions, tag):
    for c in calls:
        ok = ~(risky | c["risky"])
        got = {key: c["res"][key].cpu().numpy() for key in ("reward", "done", "returns")}
        assert got["reward"].dtype == np.int8 and got["done"].dtype == np.uint8 and got["reward"].shape == (c["T"], ok.size)
        for key in ("reward", "done"):
            np.testing.assert_array_equal(got[key][:, ok], c[key][:, ok], err_msg=f"{tag}: {key} log of tape call {c['slot']}")
        np.testing.assert_array_equal(got["returns"][ok], c["returns"][ok], err_msg=f"{tag}: returns of tape call {c['slot']}")
    for a, b in pairs:
        for key in ("reward", "done", "returns"):
            np.testing.assert_array_equal(a["res"][key].cpu().numpy(), b["res"][key].cpu().numpy(), err_msg=f"{tag}: {key}")
    assert eng.bad_action_count() == bad_actions, tag


def _assert_exercised(mir, k):
    s = mir.stats
    print(f"[view-writes] n={mir.n} K={k}: {s}, guard-band share {s['guarded'] / max(1, s['env_steps']):.5f}")
    assert s["guarded"] < 0.01 * s["env_steps"], s           # (the oracle alone: 0.09-0.23 % for this recipe)
    assert s["picked"] > 0 and s["grounded"] > 0 and s["airborne"] > 0, s
    if k <= 3:
        assert s["dones"] > 0, s


# ---- the scripts ---------------------------------------------------------------------------------------------------------
def script_state(mir):
    """GOALS / POINTS / ALIVE / ACTIONS written in front of every consumer.  Every segment is: a library call (no wait), the
    torch writes, the consumer, a checkpoint."""
    t = 0
    mir.take_views(*VIEW_FIELDS)
    mir.step_random(t)                                       # whole-degree poses, targets as drawn
    t += 1
    # step_random: fractional pose, targets moved next to where the step ends
    mir.edit_goals("fractional")
    mir.edit_points_near(mir._actions(t))
    mir.step_random(t)
    t += 1
    mir.check(label="step_random")
    # rollout(7), twice (a launch per step is a replayed graph from the second request of a length)
    for kind in ("turns", "fractional"):
        mir.rollout(2, t)
        t += 2
        mir.edit_alive()
        mir.edit_goals(kind)
        mir.edit_points_near(mir._actions(t))
        mir.rollout(7, t)
        t += 7
        mir.check(label=f"rollout(7) from {kind} poses")
    # rollout_fused(5), without and with the in-kernel re-arm
    for auto_reset, kind in ((False, "whole"), (True, "turns")):
        mir.step_random(t)
        t += 1
        mir.edit_alive()
        mir.edit_goals(kind)
        mir.edit_points_near(mir._actions(t))
        mir.rollout_fused(5, t, auto_reset=auto_reset)
        t += 5
        mir.check(label=f"rollout_fused(5, auto_reset={auto_reset}) from {kind} poses")
    # step() behind an ACTIONS write: fractional actions, a slice of them beyond +-180
    for kind in ("turns", "fractional"):
        mir.step_random(t)
        t += 1
        act = mir.rng.uniform(-179.0, 179.0, size=(mir.n, mir.dof))
        far = slice(mir.n // 3, mir.n // 3 + mir.n // 8)
        act[far] = np.where(mir.rng.rand(mir.n // 8, mir.dof) < 0.5, -1.0, 1.0) * mir.rng.uniform(180.5, 720.0, size=(mir.n // 8, mir.dof))
        act = act.astype(np.float32)
        mir.edit_alive()
        mir.edit_goals(kind)
        mir.edit_points_near(act)
        mir.step_staged(act)
        mir.check(label=f"step() from {kind} poses")
    # observe / check_done / joints_coordinates at a pose only torch wrote
    for kind in ("turns", "fractional"):
        mir.step_random(t)
        t += 1
        mir.edit_alive()
        mir.edit_goals(kind)
        mir.edit_points_near(mir.ora.goals)
        mir.observe()
        mir.check("observe", label=f"observe at {kind} poses")
        mir.step_random(t)
        t += 1
        mir.edit_goals(kind)
        mir.edit_points_near(mir.ora.goals)
        mir.edit_alive()
        mir.check_done()
        mir.check("check_done", label=f"check_done at {kind} poses")
        mir.step_random(t)
        t += 1
        mir.edit_goals(kind)
        want = mir.joints_of(mir.ora.goals)
        mir.program.append(("call", lambda e, want=want: _assert_joints(e, want)))
        mir.check("joints", label=f"joints_coordinates at {kind} poses")


def _assert_joints(eng, want):
    err = np.abs(eng.joints_coordinates() - want).max()
    assert err <= POS_TOL, err


def script_returns(mir):
    """TOTAL_REWARD.add_(bonus) in front of every consumer of the returns, over three episodes of a learner's loop: the
    overlapped gather of EVERY episode (the first one allocates the snapshot rows, so a stale snapshot can only show from the
    second), reset_random between them (-> last_return) and the next episode's rollout, which accumulates onto a bonus written
    behind that reset; in the first episode also the in-line gather, return_stats and reset_done (-> ring).  The episodes are
    6, 3 and 2 steps long: where five steps run per launch that is five + one, and twice a launch that is first and last at
    once (the oracle's steps are what a case costs, 300 007 arms included, so no episode is longer than it has to be)."""
    t = 0
    mir.take_views(*VIEW_FIELDS)
    for ep, length in enumerate((6, 3, 2)):
        if ep:
            mir.reset_random(ep)                             # own stream: deferred into the rollout below; the write's sync flushes it
        mir.edit_bonus()                                     # onto zeroed returns, behind the reset
        mir.rollout(length, t)                               # accumulates onto the bonus; its last launch may write the snapshot
        t += length
        without = mir.edit_bonus()
        mir.gather("begin", without)
        mir.check(label=f"episode {ep}: rollout({length}) on edited returns, gather_begin")   # (and last_return of the reset before)
        if ep == 0:
            # in-line gather
            mir.rollout(2, t)
            t += 2
            without = mir.edit_bonus()
            mir.gather("returns", without)
            mir.check(label="gather_returns")
            # return_stats: every env counts, so the call in front of the write is one that decides nothing
            mir.observe()
            without = mir.edit_bonus()
            mir.gather("stats", without)
            # reset_done: the finished returns, bonus included, go to the ring
            mir.edit_kill(4)
            mir.step_random(t)                               # every fourth env finishes here (no targets left)
            t += 1
            without = mir.edit_bonus()
            fin = mir.done == 1
            assert fin.sum() >= mir.n // 4 and (mir.ora.total_reward != without)[fin].mean() > 0.9
            mir.reset_done()
            mir.check("reset", label="reset_done")
        # reset_random: last_return is the edited value (checked behind the next episode's rollout, or right here at the end)
        lead = 2 if ep == 0 else 1
        mir.rollout(lead, t)
        t += lead
        without = mir.edit_bonus()
        assert (mir.ora.total_reward != without).mean() > 0.9
    mir.reset_random(3)
    mir.check("reset", label="last reset_random")


def script_points_mid_run(mir):
    """The POINTS view is taken mid-run, behind steps that ran on valid target codes: from the hand-out on the kernels have to
    read the floats."""
    t = 0
    mir.rollout(2, t)
    t += 2
    mir.step_random(t)
    t += 1
    mir.take_views("F_POINTS")
    mir.edit_points_near(mir._actions(t))
    mir.rollout(3, t)
    t += 3
    mir.check(label="rollout(3) behind the hand-out of the POINTS view")
    mir.rollout(2, t)
    t += 2
    mir.edit_points_near(mir._actions(t))
    mir.step_random(t)
    t += 1
    mir.check(label="step_random behind a second POINTS write")


def _run(m, monkeypatch, regime, script, on_torch_stream):
    eng, mir = _make(m, monkeypatch, regime, on_torch_stream)
    script(mir)
    replay(m, eng, mir, on_torch_stream)
    _assert_exercised(mir, REGIMES[regime]["k"])
    eng.close()


@pytest.mark.parametrize("regime", ["k5_lanes4", "k5_lanes2", "graph", "two_chains"])
def test_state_written_through_views_on_torch_stream_is_seen_by_every_consumer(m, monkeypatch, regime):
    _run(m, monkeypatch, regime, script_state, True)


@pytest.mark.parametrize("regime", ["k5_lanes4", "k5_lanes2", "graph", "two_chains", "large"])
def test_returns_written_through_the_view_on_torch_stream_reach_every_consumer(m, monkeypatch, regime):
    """gather_begin on the second and third episode is the case a snapshot written by mt_rollout's last launch got wrong on a
    caller's stream: the row copy was skipped and the buffer held the returns from before the torch write."""
    _run(m, monkeypatch, regime, script_returns, True)


def test_points_view_taken_mid_run_ends_the_target_codes(m, monkeypatch):
    _run(m, monkeypatch, "large", script_points_mid_run, True)


@pytest.mark.parametrize("script", [script_state, script_returns], ids=["state", "returns"])
@pytest.mark.parametrize("regime", ["k5_lanes4", "two_chains"])
def test_own_stream_control_with_the_headers_syncs_around_every_write(m, monkeypatch, regime, script):
    """The same programs on the handle's private stream, eng.sync() before and torch.cuda.synchronize() after every write.
    In the returns script a reset_random that the handle DEFERRED into the next rollout sits in front of a write: that sync
    has to launch it, or the rollout's first launch would wipe the bonus."""
    _run(m, monkeypatch, regime, script, False)


def test_dispatch_json_survives_an_override_with_a_quote_and_a_backslash(m, monkeypatch):
    """mt_describe_dispatch reports the overrides as parsed, never the raw text of the variable."""
    monkeypatch.setenv("MT_GATHER_THROTTLE", '1"\\')
    eng = m.StepEngine(64, 2)
    d = eng.dispatch()                                       # json.loads inside
    assert "MT_GATHER_THROTTLE=1" in d["overrides"].split(","), d["overrides"]
    eng.close()
