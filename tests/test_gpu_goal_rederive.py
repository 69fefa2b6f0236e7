"""GPU tests of the re-derived previous pose: a sampled step launch stores goals = its action draw, so the next one -- same
seed, next step index -- draws that pose again instead of loading it, and the first one after a full reset starts from the
zero pose without a load (kernels.h PREV; the host's record of the row: engine_internal.h GoalsRow).  A default handle and a
handle created under MT_GOALS_REDERIVE=0 (every launch loads) run the same scripts and must agree bit for bit in every field
-- across the calls that keep the record (full resets, sampled step launches with consecutive indices) and everything that
ends it (a gap in the index, another seed, mt_set, staged steps, the fused rollout, checkpoint restore, the re-arm of finished
envs, a view of the row).

Sizes: 300 007 is the default two-chain form with a ragged last block -- by default the launches of its first chain re-derive
and those of the second load (the dispatch policy's rederive_goals_chains), under MT_GOALS_REDERIVE=1 both do --, 70 001
under MT_ROLLOUT_K=1 MT_GRAPH=0 the one-chain launch-per-step form above the lane-split threshold.  The 7-joint table's rows
are built but off by the dispatch policy (they lose a wave per SIMD and measured slower): MT_GOALS_REDERIVE=1 turns them on
for the same check.  That the launches really re-derive is read from the library's own count of such launches
(dispatch()["goals"]["launches_rederived"]), not from the configuration."""
import numpy as np
import pytest

from parity_util import GUARD, POS_TOL, assert_obs_close

pytestmark = pytest.mark.gpu

FIELDS = ("F_GOALS", "F_ALIVE", "F_TOTAL_REWARD", "F_POINTS", "F_EPISODES", "F_LAST_RETURN", "F_OBS", "F_REWARD", "F_DONE",
          "F_EE", "F_DONE_BITS", "F_RETURN_RING")
SEED = 0x60A1
TOL = 30.0  # a wide pickup box: targets get picked, and envs finish, within an episode

# name -> (n, K, table, MT_* overrides, the rollout form dispatch() must report, MT_GOALS_REDERIVE of the re-deriving engine)
REGIMES = {
    "chains_k7": (300007, 7, "ref", {}, "chained_steps", None),
    "all_chains_k7": (300007, 7, "ref", {}, "chained_steps", "1"),
    "chains_k1": (300007, 1, "ref", {}, "chained_steps", None),
    "one_chain_k7": (70001, 7, "ref", {"MT_ROLLOUT_K": "1", "MT_GRAPH": "0"}, "launch_per_step", None),
    "one_chain_k1": (70001, 1, "ref", {"MT_ROLLOUT_K": "1", "MT_GRAPH": "0"}, "launch_per_step", None),
    # (the 7-joint table's launches take the prefetch kernel up to 131 072 envs only: the same one-chain form)
    "dh7_k7": (70001, 7, "dh7", {"MT_ROLLOUT_K": "1", "MT_GRAPH": "0"}, "launch_per_step", "1"),
}


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32) if v.dtype == np.float32 else v


def assert_same(m, got, want, what):
    for f in FIELDS:
        a, b = got.get(getattr(m.lib, f)), want.get(getattr(m.lib, f))
        assert a.dtype == b.dtype, (what, f)
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"{what}: {f}")


def pair(m, monkeypatch, regime):
    """(default engine, MT_GOALS_REDERIVE=0 engine) of a regime; the overrides are read once, by mt_create."""
    n, k, table, env, form, force = REGIMES[regime]
    tbl, radius = {"ref": (m.REF_DH_TABLE, 51.3), "dh7": (m.DH7_TABLE, 92.6)}[table]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    monkeypatch.delenv("MT_GOALS_REDERIVE", raising=False)
    if force is not None:
        monkeypatch.setenv("MT_GOALS_REDERIVE", force)
    on = m.StepEngine(n, k, dh_table=tbl, radius=radius, pickup_tol=TOL)
    monkeypatch.setenv("MT_GOALS_REDERIVE", "0")
    off = m.StepEngine(n, k, dh_table=tbl, radius=radius, pickup_tol=TOL)
    monkeypatch.delenv("MT_GOALS_REDERIVE", raising=False)
    d_on, d_off = on.dispatch(), off.dispatch()
    assert d_on["rollout"]["form"] == form and d_off["rollout"]["form"] == form, (d_on["rollout"], d_off["rollout"])
    assert d_on["goals"]["rederive"] is True and d_off["goals"]["rederive"] is False, (d_on["goals"], d_off["goals"])
    assert "MT_GOALS_REDERIVE=0" in d_off["overrides"]
    assert ("MT_GOALS_REDERIVE" not in d_on["overrides"]) if force is None else (f"MT_GOALS_REDERIVE={force}" in d_on["overrides"])
    chains = d_on["chains"]["count"]
    assert d_on["goals"]["chains_rederiving"] == (chains if force == "1" else min(chains, d_on["policy"]["rederive_goals_chains"]))
    # nothing else differs between the two
    for key in ("step", "chains", "rollout", "ground_compact"):
        assert d_on[key] == d_off[key], key
    return on, off


def rederived(e):
    """Step launches of this engine that took the zero pose or the draw instead of the load, so far: counted where the
    launch is made, not where the dispatch is described."""
    return e.dispatch()["goals"]["launches_rederived"]


def run_pair(m, monkeypatch, regime, script):
    on, off = pair(m, monkeypatch, regime)
    try:
        for e in (on, off):
            script(e)
            e.sync()
        assert rederived(on) > 0 and rederived(off) == 0, (script.__name__, rederived(on), rederived(off))
        assert_same(m, on, off, f"{regime} {script.__name__}")
    finally:
        on.close()
        off.close()


def episodes(e, first, count, steps=20):
    for ep in range(first, first + count):
        e.reset_random(SEED, ep)
        e.rollout(steps, SEED, ep * steps)


@pytest.mark.parametrize("regime", list(REGIMES))
def test_episodes_then_rearm(m, monkeypatch, regime):
    on, off = pair(m, monkeypatch, regime)
    try:
        for ep in range(3):
            for e in (on, off):
                episodes(e, ep, 1)
                e.sync()
            assert_same(m, on, off, f"{regime} episode {ep}")
        # every step launch of every chain that re-derives did: 20 per episode (one over the whole batch counts once)
        assert rederived(off) == 0 and rederived(on) == 3 * 20 * max(1, on.dispatch()["goals"]["chains_rederiving"])
        pts = on.points()
        assert (pts == 0).all(axis=2).any() and on.done().any()  # targets were picked and zeroed, envs finished
        for e in (on, off):
            e.reset_done(SEED)
            e.rollout(7, SEED, 100)
            e.sync()
        assert_same(m, on, off, f"{regime} reset_done")
    finally:
        on.close()
        off.close()


@pytest.mark.parametrize("regime", ["chains_k7", "all_chains_k7", "one_chain_k7"])
def test_rollout_split_over_calls(m, monkeypatch, regime):
    def consecutive(e):
        e.reset_random(SEED, 0)
        e.rollout(3, SEED, 0)
        e.rollout(4, SEED, 3)     # continues the record
        before = rederived(e)
        e.rollout(1, SEED, 7)     # a single step: one launch over the whole batch
        assert rederived(e) - before == (1 if e.dispatch()["goals"]["rederive"] else 0)
        e.rollout(2, SEED, 8)

    def gap_in_the_index(e):
        e.reset_random(SEED, 0)
        e.rollout(3, SEED, 0)
        e.rollout(4, SEED, 5)     # not the step after the last one: a load
        e.rollout(2, SEED, 0)     # nor is step 0 after any
        before = rederived(e)
        e.rollout(1, SEED, 7)     # one launch, behind step 1
        assert rederived(e) == before

    def another_seed(e):
        e.reset_random(SEED, 0)
        e.rollout(3, SEED, 0)
        e.rollout(4, SEED + 1, 3)  # the right index of another stream: a load
        before = rederived(e)
        e.rollout(1, SEED, 7)      # one launch with the index after the last one, of the first seed again
        assert rederived(e) == before
        e.rollout(3, SEED, 8)

    for script in (consecutive, gap_in_the_index, another_seed):
        run_pair(m, monkeypatch, regime, script)


@pytest.mark.parametrize("regime", ["chains_k7", "all_chains_k7", "one_chain_k7"])
def test_writers_that_end_the_record(m, monkeypatch, regime):
    n = REGIMES[regime][0]
    rng = np.random.default_rng(11)
    poses = rng.integers(-180, 180, size=(n, 4)).astype(np.float32)
    poses[1::2] += rng.uniform(-0.5, 0.5, size=poses[1::2].shape).astype(np.float32)   # whole and fractional degrees
    acts = rng.integers(-180, 180, size=(n, 4)).astype(np.float32)
    acts[::5, 1] = np.nan                                                              # unusable: those envs hold their pose

    def set_goals(e):
        episodes(e, 0, 1, steps=3)
        e.set(m.lib.F_GOALS, poses)
        e.rollout(4, SEED, 3)

    def staged_step(e):
        episodes(e, 0, 1, steps=3)
        e.step(acts)
        e.rollout(4, SEED, 3)

    def fused(e):
        episodes(e, 0, 1, steps=3)
        e.rollout_fused(5, SEED, 3, auto_reset=True)
        e.rollout(4, SEED, 3)     # the index after the last step LAUNCH: the record of that launch must be gone

    def restore(e):
        episodes(e, 0, 1, steps=6)
        st = e.get_state()
        e.rollout(5, SEED, 6)
        e.set_state(st)
        e.rollout(5, SEED, 11)    # the index after the last launch, but the pose of step 5

    def rearm(e):
        episodes(e, 0, 1, steps=12)
        e.reset_done(SEED)
        e.rollout(4, SEED, 12)

    def reset_while_forked(e):
        e.reset_random(SEED, 0)
        e.rollout(5, SEED, 0)      # (two chains: leaves them forked)
        e.reset_random(SEED, 1)    # one reset per chain, behind that chain's last step
        e.rollout(5, SEED, 5)
        e.reset_done(SEED)
        e.rollout(5, SEED, 10)

    for script in (set_goals, staged_step, fused, restore, rearm, reset_while_forked):
        run_pair(m, monkeypatch, regime, script)


def test_view_of_the_row_ends_it_for_good(m, monkeypatch):
    import torch
    n = REGIMES["all_chains_k7"][0]
    poses = torch.from_numpy(np.random.default_rng(5).integers(-180, 180, size=(4, n)).astype(np.float32) + 0.25)

    def view_write(e):
        episodes(e, 0, 1, steps=3)
        e.sync()
        e.device_ptr(m.lib.F_GOALS)
        assert e.dispatch()["goals"]["rederive"] is False
        e.use_torch_stream()
        view = e.device_tensor(m.lib.F_GOALS)
        e.rollout(2, SEED, 3)
        view.copy_(poses.to(view.device), non_blocking=True)   # between two library calls, in stream order
        e.rollout(3, SEED, 5)
        torch.cuda.synchronize()

    run_pair(m, monkeypatch, "all_chains_k7", view_write)


def test_lockstep_with_the_fp64_oracle(m, monkeypatch):
    """Ten steps of the default two-chain form at n = 300 007, two per call, against oracle.BatchOracle in fp64 with
    parity_util's tolerances.  Envs are independent, so the oracle plays a sample of them: the first and the last blocks (the
    ragged one), both sides of the chain boundary and a stride over the rest."""
    from oracle import manytor_oracle as mo
    from oracle import philox_ref as px
    n, k = REGIMES["chains_k7"][:2]
    monkeypatch.setenv("MT_GOALS_REDERIVE", "1")     # both chains re-derive
    eng = m.StepEngine(n, k, pickup_tol=TOL)
    monkeypatch.delenv("MT_GOALS_REDERIVE", raising=False)
    try:
        d = eng.dispatch()
        assert d["goals"]["rederive"] is True and d["rollout"]["form"] == "chained_steps"
        assert d["goals"]["chains_rederiving"] == d["chains"]["count"] == 2
        span = d["chains"]["span"]
        sample = np.unique(np.concatenate([np.arange(512), np.arange(span - 512, span + 512), np.arange(n - 512, n),
                                           np.arange(0, n, 37)]))
        ids = sample.astype(np.uint64)
        eng.reset_random(SEED, 0)
        ora = mo.BatchOracle(len(sample), k, pickup_tol=TOL)
        ora.reset(eng.points()[sample].astype(np.float64))
        ever_guarded = np.zeros(len(sample), dtype=bool)
        for t in range(0, 10, 2):
            eng.rollout(2, SEED, t)
            pre_alive = ora.alives.copy()
            ora.step(px.sample_actions(SEED, ids, t, 4).astype(np.float64))
            pm = np.where(pre_alive, ora.pickup_margin, np.inf).min(axis=1)
            ever_guarded |= (ora.ground_margin < GUARD) | (pm < GUARD)
            act = px.sample_actions(SEED, ids, t + 1, 4)
            pre_alive = ora.alives.copy()
            obs_ref, rew_ref, done_ref = ora.step(act.astype(np.float64))
            pm = np.where(pre_alive, ora.pickup_margin, np.inf).min(axis=1)
            ever_guarded |= (ora.ground_margin < GUARD) | (pm < GUARD)
            ok = ~ever_guarded
            np.testing.assert_array_equal(eng.goals()[sample], act)
            assert np.abs(eng.ee()[sample] - ora.joints_coordinates[:, -1]).max() <= POS_TOL
            np.testing.assert_array_equal(eng.reward()[sample][ok], rew_ref[ok])
            np.testing.assert_array_equal(eng.done()[sample][ok], done_ref[ok])
            np.testing.assert_array_equal(eng.alives()[sample][ok], ora.alives[ok])
            np.testing.assert_array_equal(eng.total_reward()[sample][ok], ora.total_reward[ok].astype(np.float32))
            assert_obs_close(eng.obs()[sample][ok], obs_ref[ok], ora.joints_coordinates[ok, -2], ora.points[ok], pre_alive[ok])
        # the comparison is not vacuous: an env-step lands in a guard band of 2e-3 around one of its 3 K + 1 thresholds with
        # a probability of the order of (3 K + 1) * 2e-3 / 50 (coordinates spread over +-50), 1e-3; ten steps: about 1 %
        assert ever_guarded.mean() < 0.1
    finally:
        eng.close()
