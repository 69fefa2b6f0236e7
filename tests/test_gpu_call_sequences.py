"""Mixed call sequences against a cache-free twin and the fp64 oracle.

The handle keeps facts on the host about what device memory holds -- the target codes match MT_F_POINTS (codes_valid), the
pose row is the zero pose or an action draw (GoalsRow), every angle is a whole degree (kFlagWholeGoals), a full reset is still
to be launched (reset_pending), the chains are forked / the gather's snapshot is current (forked, snap_valid) -- and the
kernels take shortcuts while they hold.  Every entry point that writes a pose, a target or a return has to end the right
ones; a stale one faults nothing, the next sampled step just reads last episode's codes or a table sine for a fractional
angle.  So: every Python-level entry point of StepEngine, in shuffled order, each followed by sampled steps that would use a
stale fact, each once more directly behind a reset_random (deferred where the handle defers, with the chains forked where it
forks).  tests/call_sequences.py holds the alphabet, the generator and the two followers.

Twin leg (one test per regime and shuffle): the same sequence on a second handle created under the plainest schedule
(tests/campaigns/fuzz_rollout.py's, plus MT_GOALS_REDERIVE=0) whose MT_F_POINTS and MT_F_GOALS were exposed before its first
step: it never reads a code, never trusts a pose record, never sets the whole-degree flag, defers nothing and has one chain.
After every op's trailing sampled steps the twelve fields agree bit for bit, and so does every tensor the op returned --
and, the handles being created with debug_zmin=True, MT_F_ZMIN: a table sine taken for a fractional start pose changes the
lowest z of the ground test for every env it happens to, but the reward only of the few whose ground flag it flips.  No
knob had to stay at its default in the twin: no entry point differs between the schedules.  The fields are compared on the
device (mt_get into device memory, what get() does without its host copy: at 300 007 envs the copies would be the test's
time); the Python-level get() of every field is an op of the alphabet like the others.  That the handle under test really
takes its shortcuts is read from its own count of re-deriving launches, which also has to grow behind the calls that keep
the pose record (CODE_KEEPING below says where that can be asked).

Oracle leg (one test per regime, shuffle 0): the sequence in lock step with oracle.manytor_oracle.BatchOracle in fp64 on a
sample of the envs, compared after every step-producing op and after its trailing steps with parity_util's tolerances; an env
that came within GUARD of a threshold is out of the exact fields until the next full reset, and fewer than 10 % are at any
comparison (tests/test_call_sequences_host.py knows that before a GPU is involved).

Which leg holds which op:
  both    step(host actions), set_actions(device)+step, sample_actions+step, step_host, step_random, env_step,
          env_reset(points), env_reset(None), reset(points), reset_done, rollout_fused (both), rollout_actions (both),
          shoot(commit=H) (the plan rows best[i]), cem(commit=H) and mppi(commit=H) (their `chosen` output names the committed
          angles), rollout_policy (both; its action log: the dynamics under a policy, the MLP is held by test_gpu_policy.py),
          rollout_population (its action log), set(F_GOALS / F_POINTS / F_ALIVE), set_state, observe and check_done (the
          oracle repeats them: get_observations / is_done), ik(stage)+step (its `angles` output names the staged angles; an
          env it held is handed its own pose)
  twin    es: no output of the call names the actions it committed, so it is left out of the oracle leg's sequence
  twin, and the handle against itself (fields before == fields after the op)
          rollout_actions(dry_run=True), shoot / cem / mppi(commit=0), sample_plans, sample_population, policy_eval,
          policy_grad, value_grad, gae, reward_to_go, bad_action_count, get, sync, return_stats, gather_begin+gather_wait,
          gather_returns, lap_begin+lap_end, dispatch; the oracle leg runs them too, as calls between its steps.
  twin, the handle against itself, and tests/ik_ref.py in fp64 on the oracle's own pose, targets and alive mask
          jacobian, ik -- and the ik half of ik(stage)+step, ahead of its step (compare_ik_with_reference)
Two of the "change nothing" ops are recomputations, not no-ops, and are held as such: observe rewrites MT_F_OBS from the
state AFTER the pickups (a target picked in the last step reads 0 where the step's observation, taken before the pickup,
had a distance) and zeroes the coordinates of dead targets (manytor.py:148); check_done repeats the pickup test, which right
after a reset picks what lies within the box of the zero pose, and behind a step may differ from the step's own test for a
target within rounding of the box's face (its kernel computes the pose by another route).  Everything else is unchanged
across them, and those fields change only in these ways.  Directly behind a reset_random a snapshot from before the op would
launch the deferred reset, so there the fields after the op are held to what a full reset leaves: zero pose, all alive, zero
returns and flags, the episode index, the targets of (seed, env, episode) from philox_ref.
"""
import numpy as np
import pytest

import call_sequences as cs
import ik_ref
from parity_util import DIST_TOL, GUARD, POS_TOL, assert_obs_close

pytestmark = pytest.mark.gpu

PER_STEP = {"MT_ROLLOUT_K": "1", "MT_GRAPH": "0"}
# name -> (n, MT_* overrides, on torch's stream)
REGIMES = {
    "split": (5003, {}, False),
    "multi": (70001, {}, False),
    "per_step": (70001, PER_STEP, False),
    "two_chain_multi": (200003, {}, False),
    "chains": (300007, {}, False),
    "chains_all": (300007, {"MT_GOALS_REDERIVE": "1"}, False),
    "chains_torch": (300007, {}, True),
    "pop_per_step": (70144, PER_STEP, False),
    "pop_chains": (300032, {}, False),
}
REDERIVING = ("per_step", "chains", "chains_all", "pop_per_step", "pop_chains")
TWIN_ENV = {"MT_CHAINS": "1", "MT_GRAPH": "0", "MT_TRIG_TABLE": "0", "MT_SPLIT": "0", "MT_PREFETCH": "0", "MT_RESET_SPLIT": "0",
            "MT_LAZY_CHAINS": "0", "MT_ROLLOUT_K": "1", "MT_ROLLOUT_EARLY": "0", "MT_DEFER_RESET": "0", "MT_ROLLOUT_SNAP": "0",
            "MT_DEFER_RESET_CHAINS": "0", "MT_GOALS_REDERIVE": "0"}
SHUFFLES = (0, 1, 2)
CAP = 0.10
# The pose is re-derived by the code-reading step kernels only (kernels.h: PREV needs CODES), and the codes come back with a
# full random reset alone.  So the sampled steps behind an op are REQUIRED to re-derive where every op since the last
# reset_random was one of these -- calls that change nothing, the sampled step, the re-arm (it writes the codes it draws);
# each op's appearance directly behind a reset_random is such a place.  Elsewhere a load is not a defect and nothing is asked.
CODE_KEEPING = cs.NOTHING + ("step_random", "reset_done")

_DATA = {}


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def data_for(n, span):
    if (n, span) not in _DATA:
        _DATA.clear()                    # one batch size's arrays at a time
        _DATA[n, span] = cs.Data(n, span)
    return _DATA[n, span]


def create(m, monkeypatch, env, n):
    for key in TWIN_ENV:
        monkeypatch.delenv(key, raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    e = m.StepEngine(n, cs.K, pickup_tol=cs.TOL, return_ring=cs.RING, debug_zmin=True)   # the overrides are read once, by mt_create
    for key in env:
        monkeypatch.delenv(key, raising=False)
    return e


def engine_of(m, monkeypatch, regime):
    """The handle under test; its dispatch form asserted from dispatch(), not from the size."""
    n, env, on_torch = REGIMES[regime]
    e = create(m, monkeypatch, env, n)
    d = e.dispatch()
    r, ch, g = d["rollout"], d["chains"], d["goals"]
    if regime == "split":
        assert d["step"]["lanes_per_env"] == 4 and d["reset"]["lanes_per_env"] == 4, d
        assert r["form"] == "multi_step" and r["steps_per_launch"] > 1 and r["absorbs_reset"] is True, r
    elif regime == "multi":
        assert d["step"]["lanes_per_env"] == 1 and ch["count"] == 1, d
        assert r["form"] == "multi_step" and r["steps_per_launch"] > 1 and r["absorbs_reset"] is True, r
    elif regime in ("per_step", "pop_per_step"):
        assert r["form"] == "launch_per_step" and ch["count"] == 1 and g["rederive"] is True and g["step"] is True, d
    elif regime == "two_chain_multi":
        assert ch["count"] == 2 and ch["lazy"] is True, ch
        assert r["form"] == "multi_step" and r["chains"] == 1 and r["absorbs_reset"] is True, r
    else:
        assert r["form"] == "chained_steps" and ch["count"] == 2 and ch["lazy"] is True and g["rederive"] is True, d
        assert g["chains_rederiving"] == (2 if regime == "chains_all" else d["policy"]["rederive_goals_chains"]), g
    if on_torch:
        e.use_torch_stream()             # every call joins, nothing is deferred
    return e, d


def twin_of(m, monkeypatch, n):
    t = create(m, monkeypatch, TWIN_ENV, n)
    t.device_ptr(m.lib.F_POINTS)         # the floats, for good
    t.device_ptr(m.lib.F_GOALS)          # ... and neither a pose record nor the whole-degree flag
    d = t.dispatch()
    assert d["rollout"]["form"] == "launch_per_step" and d["rollout"]["absorbs_reset"] is False, d["rollout"]
    assert d["chains"]["count"] == 1 and d["step"]["lanes_per_env"] == 1 and d["step"]["prefetch"] is False, d
    assert d["step"]["trig_table"] is False and d["reset"]["lanes_per_env"] == 1 and d["goals"]["rederive"] is False, d
    for key, val in TWIN_ENV.items():
        assert f"{key}={val}" in d["overrides"], (key, d["overrides"])
    return t


def rederived(e):
    return e.dispatch()["goals"]["launches_rederived"]


def bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32) if v.dtype == np.float32 else v


def same_bits(x, y):
    """Two device tensors hold the same bits."""
    import torch
    if x.dtype != y.dtype or x.shape != y.shape:
        return False
    if x.dtype == torch.float32:
        x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
    return torch.equal(x, y)


def assert_same_fields(a, b, what, skip=(), zmin_exact=True):
    """Two snapshots (cs.Runner.snapshot: device tensors) agree bit for bit; zmin_exact=False: MT_F_ZMIN within 2 POS_TOL."""
    if not zmin_exact:
        skip = tuple(skip) + ("F_ZMIN",)
        worst = float((a["F_ZMIN"] - b["F_ZMIN"]).abs().max())
        assert worst <= 2 * POS_TOL, f"{what}: F_ZMIN differs by {worst}"
    for f in cs.SNAP_FIELDS:
        if f not in skip and not same_bits(a[f], b[f]):
            x, y = a[f].cpu().numpy(), b[f].cpu().numpy()
            np.testing.assert_array_equal(bits(x), bits(y), err_msg=f"{what}: {f}")
            raise AssertionError(f"{what}: {f}")


def assert_same_outputs(a, b, what):
    import torch
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, torch.Tensor):
            assert same_bits(x, y), f"{what}: output {key}"
        elif isinstance(x, np.ndarray):
            np.testing.assert_array_equal(bits(x), bits(y), err_msg=f"{what}: output {key}")
        else:
            assert x == y, (what, key, x, y)


def dead_and_finished(snap):
    return bool((snap["F_POINTS"] == 0).all(dim=2).any()), bool(snap["F_DONE"].any())


def near_the_box(snap):
    """(N, K): the end effector is within rounding (2 POS_TOL) of a face of the target's pickup box."""
    delta = np.abs(snap["F_EE"][:, None, :].astype(np.float64) - snap["F_POINTS"])
    return np.abs(delta - cs.TOL).min(axis=-1) < 2 * POS_TOL


def assert_unchanged(op, before, after, what):
    """A "changes nothing" op on the handle itself: the fields after it against the fields before it."""
    if op not in ("observe", "check_done"):
        return assert_same_fields(before, after, what)
    skip = ("F_OBS", "F_POINTS") if op == "observe" else ("F_ALIVE", "F_DONE", "F_DONE_BITS")
    assert_same_fields(before, after, what, skip=skip)
    before, after = cs.to_host(before), cs.to_host(after)
    if op == "observe":
        alive = before["F_ALIVE"].astype(bool)
        np.testing.assert_array_equal(bits(after["F_POINTS"][alive]), bits(before["F_POINTS"][alive]), err_msg=what)
        assert (after["F_POINTS"][~alive] == 0).all(), what
        obs0, obs1 = (s["F_OBS"].reshape(alive.shape + (3,)) for s in (before, after))
        assert (obs1[~alive] == 0).all(), what
        # the same distance by another kernel: both within DIST_TOL of the exact one
        assert np.abs(obs1[..., 0] - obs0[..., 0])[alive & (obs0[..., 0] != 0)].max(initial=0.0) <= 2 * DIST_TOL, what
    else:
        a0, a1 = before["F_ALIVE"].astype(bool), after["F_ALIVE"].astype(bool)
        assert not (a1 & ~a0).any(), what
        assert not ((a0 != a1) & ~near_the_box(before)).any(), what
        touched = (a0 != a1).any(axis=1)
        np.testing.assert_array_equal(after["F_DONE"][~touched], before["F_DONE"][~touched], err_msg=what)
        np.testing.assert_array_equal(after["F_DONE"] != 0, ~a1.any(axis=1), err_msg=what)


def assert_fresh(m, op, after, g, points_ref, sample, what):
    """The fields behind `reset_random(SEED, ep); op` for an op that changes nothing: what a full reset leaves."""
    after = cs.to_host(after)
    assert (after["F_GOALS"] == 0).all() and (after["F_TOTAL_REWARD"] == 0).all() and (after["F_REWARD"] == 0).all(), what
    assert (after["F_EPISODES"] == g.ep).all(), what
    if op != "check_done":               # (the pickup test at the zero pose picks what lies in its box)
        assert (after["F_ALIVE"] == 1).all() and not after["F_DONE"].any() and not after["F_DONE_BITS"].any(), what
    pts = after["F_POINTS"][sample]
    live = after["F_ALIVE"][sample].astype(bool)
    np.testing.assert_array_equal(bits(pts[live]), bits(points_ref[live]), err_msg=what)
    if op == "observe":
        assert (pts[~live] == 0).all(), what


def check_own_returns(op, out, after, n, what):
    """gather_* and return_stats against get(F_TOTAL_REWARD) of the same handle."""
    if "gather" in op:
        assert same_bits(out["gathered"], after["F_TOTAL_REWARD"]), what
    elif op == "return_stats":
        tot = after["F_TOTAL_REWARD"].cpu().numpy()
        assert out["count"] == n and out["sum"] == tot.astype(np.float64).sum(), (what, out)
        assert out["min"] == tot.min() and out["max"] == tot.max() and out["done"] == int(after["F_DONE"].count_nonzero()), (what, out)


@pytest.mark.parametrize("shuffle", SHUFFLES)
@pytest.mark.parametrize("regime", list(REGIMES))
def test_sequence_against_the_twin(m, monkeypatch, regime, shuffle):
    from oracle import philox_ref as px
    n = REGIMES[regime][0]
    eng, d = engine_of(m, monkeypatch, regime)
    twin = twin_of(m, monkeypatch, n)
    try:
        span = d["chains"]["span"]
        data = data_for(n, span)
        sample = cs.sample_of(n, span)
        head, groups = cs.generate(shuffle, n)
        assert sorted({g.op for g in groups}) == sorted(cs.alphabet(n))
        ra, rb = cs.Runner(m, eng, data), cs.Runner(m, twin, data)
        for r in (ra, rb):
            for it in head:
                r.item(it)
        last = ra.snapshot()
        # MT_F_ZMIN against the twin: bit for bit where every kernel of the handle puts one env per lane, as the twin's do.
        # Elsewhere within 2 POS_TOL: a wave that holds a lane with a route end beyond +-180 degrees (the staged angles reach
        # -180.5) evaluates all its lanes pose by pose (kernels.h, wide_route), its narrow lanes' z-minimum is then that
        # form's -- within 1e-4 of the reference, like the recurrence's -- and which envs share a wave depends on the lanes
        # per env.  (By the same text their ground flag may differ inside the guard band; the twelve fields never did.)
        exact = all(d[key]["lanes_per_env"] == 1 for key in ("step", "rollout", "fused") + (("chains",) if d["chains"]["count"] > 1 else ()))
        assert exact or regime in ("split", "multi", "per_step", "pop_per_step"), (regime, d)
        assert_same_fields(last, rb.snapshot(), f"{regime}/{shuffle} head", zmin_exact=exact)
        zeroed = finished = False
        coded = True                     # the handle may still know its target codes: see CODE_KEEPING
        for i, g in enumerate(groups):
            what = f"{regime}/{shuffle} #{i} {'reset_random; ' if g.with_reset else ''}{g.op}"
            for r in (ra, rb):
                for it in g.pre:
                    r.item(it)
            coded = (coded or any(it[0] == "reset_random" for it in g.pre)) and g.op in CODE_KEEPING
            nothing = g.op in cs.NOTHING
            moved = any(it[0] != "save_state" for it in g.pre)
            before = None if g.with_reset else (ra.snapshot() if moved else last) if nothing else None
            c0 = rederived(eng)
            out = ra.op(g)
            assert_same_outputs(out, rb.op(g), what)
            if g.op == "ik(stage)+step":   # not on held envs only
                assert float(((out["index"] >= 0) & (out["steps"] > 0)).float().mean()) >= cs.REACH_FLOOR, what
            if nothing:
                after = ra.snapshot()
                if g.with_reset:
                    ref = px.sample_targets(cs.SEED, sample.astype(np.uint64), g.ep, cs.K, cs.RADIUS)
                    assert_fresh(m, g.op, after, g, ref, sample, what)
                else:
                    assert_unchanged(g.op, before, after, what)
                check_own_returns(g.op, out, after, n, what)
            c1 = rederived(eng)
            for r in (ra, rb):
                for it in g.trail:
                    r.item(it)
            if regime in REDERIVING and coded:     # the optimisation is not lost either
                if g.op in cs.KEEPERS:
                    assert rederived(eng) > c1, (what, "the sampled steps behind a record-keeping call loaded the pose")
                if g.op == "step_random":
                    assert c1 > c0, (what, "a step_random that continues the index loaded the pose")
            last = ra.snapshot()
            assert_same_fields(last, rb.snapshot(), what, zmin_exact=exact)
            z, f = dead_and_finished(last)
            zeroed, finished = zeroed or z, finished or f
        assert zeroed and finished       # targets were picked and zeroed, envs finished
        assert rederived(twin) == 0
        if regime in REDERIVING:
            assert rederived(eng) > 0
        assert eng.bad_action_count() == twin.bad_action_count() > 0     # the unusable staged actions were met
    finally:
        eng.close()
        twin.close()


# ---- the oracle leg ----------------------------------------------------------------------------------------------------
def committed_actions(op, out, data, sample, idx):
    """(steps, m, D): the actions of the sampled envs that the call committed, from its own outputs."""
    if op == "shoot(commit=H)":
        best = out["best"].index_select(0, idx).cpu().numpy()
        plans = data.plans[:, :cs.H][..., sample]                       # (C, H, D, m)
        return plans[best, :, :, np.arange(len(sample))].transpose(1, 0, 2)
    if op == "ik(stage)+step":
        return out["angles"].index_select(1, idx).cpu().numpy().T[None]
    key = "chosen" if op in ("cem(commit=H)", "mppi(commit=H)") else "actions"
    return out[key].index_select(2, idx).cpu().numpy().transpose(0, 2, 1)


def compare_with_oracle(runner, idx, fo, what, out=None, only=None):
    s, o, L = fo.sample, fo.ora, fo.last
    assert fo.guarded.mean() < CAP, (what, fo.guarded.mean())
    sel = np.ones(len(s), dtype=bool)
    if only is not None:
        sel[:] = False
        sel[only] = True
    ok = ~fo.guarded & sel
    got = runner.rows(("F_EE", "F_REWARD", "F_DONE", "F_ALIVE", "F_TOTAL_REWARD", "F_EPISODES", "F_POINTS", "F_OBS", "F_ZMIN"),
                      idx)
    get = got.__getitem__
    assert np.abs(get("F_EE")[sel] - L["jc"][sel, -1]).max() <= POS_TOL, what       # continuous: guard band or not
    assert np.abs(get("F_ZMIN")[sel] - L["zmin"][sel]).max() <= POS_TOL, what       # ... and so is the ground test's lowest z
    np.testing.assert_array_equal(get("F_REWARD")[ok], L["rew"][ok], err_msg=what)
    np.testing.assert_array_equal(get("F_DONE")[ok] != 0, L["done"][ok], err_msg=what)
    alive = get("F_ALIVE").astype(bool)
    np.testing.assert_array_equal(alive[ok], o.alives[ok], err_msg=what)
    np.testing.assert_array_equal(get("F_TOTAL_REWARD")[ok], o.total_reward[ok].astype(np.float32), err_msg=what)
    np.testing.assert_array_equal(get("F_EPISODES")[ok], fo.episodes[ok], err_msg=what)
    live = o.alives & ok[:, None]
    np.testing.assert_array_equal(get("F_POINTS")[live], o.points.astype(np.float32)[live], err_msg=what)
    assert_obs_close(get("F_OBS")[ok], L["obs"][ok], L["jc"][ok, -2], L["points"][ok], L["pre_alive"][ok])
    if out and fo.log and getattr(out.get("reward"), "ndim", 0) == 2:   # the per-step logs and the call's return, where given
        rew = out["reward"].index_select(1, idx).cpu().numpy()
        done = out["done"].index_select(1, idx).cpu().numpy()
        for t, (r_ref, d_ref) in enumerate(fo.log):
            np.testing.assert_array_equal(rew[t][ok], r_ref[ok], err_msg=f"{what}: reward log, step {t}")
            np.testing.assert_array_equal(done[t][ok] != 0, d_ref[ok], err_msg=f"{what}: done log, step {t}")
        if "returns" in out:
            total = np.sum([r for r, _ in fo.log], axis=0)
            np.testing.assert_array_equal(out["returns"].index_select(0, idx).cpu().numpy()[ok], total[ok].astype(np.float32), err_msg=what)


def compare_jacobian_with_reference(op, out, idx, fo, what):
    """jacobian(position=True) of the resident pose against ik_ref on the oracle's pose (fp32 actions: the same numbers)."""
    ok = ~fo.guarded
    J_ref, p_ref = ik_ref.jacobian(fo.ora.goals, ik_ref.REF_TABLE)
    J = out["jacobian"].index_select(2, idx).cpu().numpy().transpose(2, 0, 1)        # (m, 3, D)
    p = out["position"].index_select(1, idx).cpu().numpy().T
    worst_j, worst_p = np.abs(J - J_ref)[ok].max(), np.abs(p - p_ref)[ok].max()
    print(f"{what}: jacobian off by {worst_j:.3e} per degree, position by {worst_p:.3e}")
    assert worst_j <= ik_ref.JAC_TOL and worst_p <= ik_ref.POS_TOL, (what, worst_j, worst_p)


def compare_ik_with_reference(op, out, idx, fo, what):
    """ik in nearest mode from the resident pose against ik_ref on the oracle's own pose, targets and alive mask, over the
    unguarded envs: for those the three rows hold the oracle's numbers exactly (poses are committed fp32 actions, targets are
    fp32 draws).  `ik`: 4 iterations, no early stop; the ik of ik(stage)+step: up to 6, stopping at a box residual of 1."""
    o = fo.ora
    staged = op == "ik(stage)+step"
    ok = ~fo.guarded
    q0 = o.goals
    angles = out["angles"].index_select(1, idx).cpu().numpy().T                      # (m, D)
    residual, steps, index = (out[key].index_select(0, idx).cpu().numpy() for key in ("residual", "steps", "index"))
    # the target: none exactly where the oracle has none alive, else an alive one within 1e-3 of the nearest (fp64 distances)
    none = ~o.alives.any(axis=1)
    np.testing.assert_array_equal((index == -1)[ok], none[ok], err_msg=what)
    live, held = np.flatnonzero(ok & ~none), ok & none
    assert (index[live] >= 0).all() and (index[live] < cs.K).all() and o.alives[live, index[live]].all(), what
    _, d2 = ik_ref.nearest(o.points, o.alives, q0, ik_ref.REF_TABLE)
    assert (np.sqrt(d2[live, index[live]]) <= np.sqrt(d2[live].min(axis=1)) + 1e-3).all(), what
    # held envs: the start pose bit for bit
    np.testing.assert_array_equal(bits(angles[held]), bits(q0[held].astype(np.float32)), err_msg=what)
    assert (residual[held] == 0).all() and (steps[held] == 0).all(), what
    # the residual reported is the box residual of the angles returned
    x = o.points[live, index[live]]
    box = ik_ref.box(x - ik_ref.position(angles[live].astype(np.float64), ik_ref.REF_TABLE))
    assert np.abs(residual[live] - box).max(initial=0.0) <= ik_ref.RESIDUAL_TOL, what
    if staged:
        assert (steps[live] <= cs.REACH_ITERS).all(), what
        early = steps[live] < cs.REACH_ITERS
        assert (residual[live][early] <= cs.REACH_TOL + ik_ref.RESIDUAL_TOL).all(), what
        share = ((index >= 0) & (steps > 0)).mean()                                  # not on held envs only
        print(f"{what}: {100 * share:.1f} % of the sample reach for a target, {100 * early.mean():.1f} % of those stopped early")
        assert share >= cs.REACH_FLOOR, (what, share)
    else:
        assert (steps[live] == cs.IK_ITERS).all() and len(live) > 0, what
        ref = ik_ref.ik(x, q0[live], ik_ref.REF_TABLE, iters=cs.IK_ITERS, wrap=True)[0]
        worst = np.abs(ik_ref.wrap180(angles[live] - ref)).max()
        print(f"{what}: angles off by {worst:.3e} degrees after {cs.IK_ITERS} iterations ({len(live)} envs)")
        assert worst <= ik_ref.SEQ_STEP_TOL, (what, worst)


@pytest.mark.parametrize("regime", list(REGIMES))
def test_sequence_in_lockstep_with_the_fp64_oracle(m, monkeypatch, regime):
    import torch
    n = REGIMES[regime][0]
    eng, d = engine_of(m, monkeypatch, regime)
    try:
        span = d["chains"]["span"]
        data = data_for(n, span)
        sample = cs.sample_of(n, span)
        idx = torch.from_numpy(sample).to(torch.device("cuda", eng.device))
        fo = cs.OracleFollower(sample, data, GUARD)
        ra = cs.Runner(m, eng, data)
        head, groups = cs.generate(0, n, oracle=True)
        for it in head:
            ra.item(it)
            fo.item(it)
        compare_with_oracle(ra, idx, fo, f"{regime} head")
        for i, g in enumerate(groups):
            what = f"{regime} #{i} {'reset_random; ' if g.with_reset else ''}{g.op}"
            for it in g.pre:
                ra.item(it)
                fo.item(it)
            out = ra.op(g)
            if g.op in ("jacobian", "ik", "ik(stage)+step"):     # ahead of the oracle's own step: on the state the call read
                (compare_jacobian_with_reference if g.op == "jacobian" else compare_ik_with_reference)(g.op, out, idx, fo, what)
            fo.op(g, lambda op: committed_actions(op, out, data, sample, idx))
            if cs.op_steps(g.op):
                compare_with_oracle(ra, idx, fo, what, out, only=fo.single if g.op == "env_step" else None)
            for it in g.trail:
                ra.item(it)
                fo.item(it)
            compare_with_oracle(ra, idx, fo, what + " + sampled steps")
        assert fo.rearmed > len(sample) // 10            # envs finished, and were re-armed with the targets philox_ref names
        if regime in REDERIVING:
            assert rederived(eng) > 0
    finally:
        eng.close()
