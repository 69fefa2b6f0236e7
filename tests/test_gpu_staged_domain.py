"""Staged actions and poses of ANY accepted magnitude, pinned to the fp64 oracle.

The library accepts a staged action or a joint angle up to +-32 768 degrees (kernels.h: unusable_angle, engine.hip:
kMaxAngleBits, include/manytor_hip.h).  The accuracy contract is unconditional -- positions and the z-minimum behind the
ground flag within POS_TOL = 1e-4 of the fp64 reference, discrete outputs exact outside the GUARD = 1e-3 band
(parity_util.py) -- but every other test stages angles within +-200 degrees.  Far out, the ulp of
an fp32 angle is up to 0.004 degrees: every fp32 sum on the way to a sine (pose + joint offset, (action - pose) / (S - 1),
pose + k * increment) rounds by more than the whole tolerance unless it is formed with care (kernels.h:
route_kinematics_wide).  Here every env of seeded populations over the whole range (staged_populations.py: wild +-A, local
moves on whole turns, a list of edge values) is compared with oracle.c_oracle.COracle, whose agreement with the other
restatements on these very populations is checked on the CPU (test_oracle_golden.py), through every step schedule, table
kind and entry point that stages or inherits such a pose.

Measured maxima are recorded through test_gpu_zmin.py's record(), into the same file."""
import numpy as np
import pytest

import staged_populations as sp
from parity_util import GUARD, POS_TOL, assert_obs_close
from test_gpu_zmin import force, record
from test_gpu_zmin import tables as zmin_tables

pytestmark = pytest.mark.gpu

POPULATIONS = ["wild180", "wild720", "wild2048", "wild8192", "wild32768", "local", "edges"]
K = 5


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def tables(m):
    t = dict(zmin_tables(m))
    t["rtfrac"] = sp.fractional_offset_table()
    return t


def amplitude(population):
    return int(population[4:]) if population.startswith("wild") else 32768


class Pair:
    """An engine and the C oracle on the same targets, brought to the same pose, stepped with the same fp32 actions."""

    def __init__(self, m, n, table, radius, substeps=25, seed=0xD0E5, **kw):
        from oracle import c_oracle
        self.m, self.n = m, n
        self.fo, self.fe = kw.get("obs_frame", -2), kw.get("ee_frame", -1)
        self.eng = m.StepEngine(n, K, dh_table=table, radius=radius, substeps=substeps, debug_zmin=True, **kw)
        self.ora = c_oracle.COracle(n, K, table=np.asarray(table), radius=radius, substeps=substeps, threads=16,
                                    obs_frame=self.fo, ee_frame=self.fe)
        self.eng.reset_random(seed, 0)
        self.ora.reset(self.eng.points().astype(np.float64))
        self.guarded = 0
        self.steps = 0
        self.clean = np.ones(n, dtype=bool)     # envs that never were inside the guard band
        self.worst = {"zmin": 0.0, "ee": 0.0, "joints": 0.0}

    def pose(self, prev):
        self.eng.set(self.m.lib.F_GOALS, prev)
        self.ora.goals[:] = prev

    def oracle_step(self, action):
        self.pre_alive = self.ora.alives.copy()
        self.ref = self.ora.step(action.astype(np.float64))

    def compare(self, action, what):
        """After eng and ora took the same step: every env, every output."""
        eng, ora = self.eng, self.ora
        obs_ref, rew_ref, done_ref = self.ref
        self.steps += 1
        errs = {"zmin": np.abs(eng.zmin() - ora.zmin),
                "ee": np.abs(eng.ee() - ora.joints_coordinates[:, self.fe]).max(axis=1),
                "joints": np.abs(eng.joints_coordinates() - ora.joints_coordinates).max(axis=(1, 2))}
        for name, err in errs.items():
            self.worst[name] = max(self.worst[name], float(err.max()))
        print(f"{what}: " + "  ".join(f"{name} {err.max():.3e} (env {int(err.argmax())})" for name, err in errs.items()))
        for name, err in errs.items():
            assert err.max() <= POS_TOL, (what, name, float(err.max()), int(err.argmax()))
        assert_obs_close(eng.obs(), obs_ref, ora.joints_coordinates[:, self.fo], ora.points, self.pre_alive)
        np.testing.assert_array_equal(eng.goals().view(np.uint32), np.ascontiguousarray(action).view(np.uint32))
        assert eng.bad_action_count() == 0
        # The guard band of the ground flag is that of the value it is the sign of, the z-minimum: |zmin| < GUARD.  (ground_margin
        # -- the smallest |z| of ANY pose -- would also set aside envs that graze z = 0 at one pose and are far underground at
        # another: 2e-3 of these many-turn routes per step, for a flag that is not in doubt.  This band is the narrower one.)
        pm = np.where(self.pre_alive, ora.pickup_margin, np.inf).min(axis=1)
        risky = (np.abs(ora.zmin) < GUARD) | (pm < GUARD)
        assert np.all(ora.ground_margin <= np.abs(ora.zmin) + 1e-12)
        ok = ~risky
        self.guarded += int(risky.sum())
        self.clean &= ok
        np.testing.assert_array_equal(eng.reward()[ok], rew_ref[ok], err_msg=what)
        np.testing.assert_array_equal(eng.done()[ok], done_ref[ok], err_msg=what)
        alive_gpu = eng.alives()
        np.testing.assert_array_equal(alive_gpu[ok], ora.alives[ok], err_msg=what)
        idx = np.flatnonzero(risky)                      # re-synchronise the few envs inside the guard band
        ora.alive_u8[idx] = alive_gpu[idx]
        ora.total_reward[idx] = eng.total_reward()[idx]
        ora.points[idx] = eng.points()[idx].astype(np.float64)
        np.testing.assert_array_equal(eng.total_reward(), ora.total_reward.astype(np.float32))
        return ok

    def staged_step(self, action, what):
        self.oracle_step(action)
        self.eng.step(action)
        return self.compare(action, what)

    def finish(self, **kw):
        # a condition on the INPUTS (the cap of test_full_size_every_env_against_the_c_oracle), not a tolerance
        assert self.guarded < self.steps * self.n * 2e-3 + 8, self.guarded
        record(kernel=self.eng.step_kernel_name(), max_err_zmin=self.worst["zmin"], max_err_ee=self.worst["ee"],
               max_err_joints=self.worst["joints"], guarded=self.guarded, **kw)


def there_and_back(m, n, table_name, population, substeps=25, test="", **kw):
    """prev -> action -> prev: two staged steps with both ends drawn from the population."""
    table, radius = tables(m)[table_name]
    prev, action = sp.make(population, 0x57A6ED + len(table), n, len(table), substeps)
    p = Pair(m, n, table, radius, substeps, **kw)
    p.pose(prev)
    ok1 = p.staged_step(action, f"{population} {table_name} out")
    p.staged_step(prev, f"{population} {table_name} back")
    p.finish(test=test, table=table_name, population=population, A=amplitude(population), S=substeps)
    return p, ok1


# ---- the staged step kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("population", POPULATIONS)
@pytest.mark.parametrize("table_name", ["ref", "dh7", "rt5", "rtfrac"])
@pytest.mark.parametrize("schedule", ["streaming", "prefetch", "split2", "split4"])
def test_staged_step_under_every_forced_schedule(m, monkeypatch, schedule, table_name, population):
    """step_kernel (streaming / prefetch) and step_split_kernel<2|4>, 262 144 envs, the compile-time tables, a runtime table
    and one whose theta offsets are not whole degrees (pose + offset rounds at the ulp of the pose)."""
    force(monkeypatch, schedule)
    p, _ = there_and_back(m, 262144, table_name, population, test="staged_schedule_" + schedule)
    want = {"streaming": "pf=0", "prefetch": "pf=8", "split2": "L=2", "split4": "L=4"}[schedule]
    assert want in p.eng.step_kernel_name(), p.eng.step_kernel_name()


@pytest.mark.parametrize("population", ["wild180", "wild2048", "wild32768", "local", "edges"])
@pytest.mark.parametrize("table_name", ["ref", "dh7"])
def test_staged_step_at_full_size_with_the_default_dispatch(m, table_name, population):
    """1 048 576 envs with whatever mt_create picks there (concurrent chains over env ranges included)."""
    there_and_back(m, 1048576, table_name, population, test="staged_default_1m")


def test_the_control_population_is_the_fractional_degree_test(m):
    """A = 180 reproduces test_gpu_zmin.test_zmin_with_fractional_degree_actions: uniform fractional actions within +-180
    on the narrow path, whose error the wide populations are to be read against."""
    prev, action = sp.wild(1, 4096, 4, 180)
    assert np.abs(prev).max() <= 180 and np.abs(action).max() <= 180 and (action != np.round(action)).mean() > 0.99


@pytest.mark.parametrize("table_name", ["ref", "dh7"])
def test_local_moves_keep_both_outcomes_of_the_ground_flag_in_play(m, table_name):
    """`wild` routes nearly all sweep through the ground; the local population is there so that a kernel that got the flag
    wrong in EITHER direction far out would be seen: each outcome holds at least 0.5 % of the envs outside the guard band."""
    n = 262144
    table, radius = tables(m)[table_name]
    prev, action = sp.make("local", 0x57A6ED + len(table), n, len(table))
    assert np.abs(prev).max() > 30000 and np.abs(action).max() > 30000
    p = Pair(m, n, table, radius)
    p.pose(prev)
    ok = p.staged_step(action, "local " + table_name)
    grounded = p.ora.ground_hit[ok].mean()
    print(f"local {table_name}: grounded share {grounded:.4f}, in guard band {int((~ok).sum())}")
    assert 0.005 <= grounded <= 0.995, grounded
    np.testing.assert_array_equal((p.eng.zmin() < 0)[ok], p.ora.ground_hit[ok])


# ---- the other instantiations of the step kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("population", ["wild2048", "wild32768", "local", "edges"])
@pytest.mark.parametrize("form", ["frames25", "frames40", "direct64", "lds"])
def test_staged_step_of_the_other_kernel_forms(m, form, population):
    """RtTableF (selectable frames) with the recurrence (S = 25) and with the per-pose form (S = 40); direct_trig at S = 64
    (a long route); the table in LDS."""
    substeps, kw, want = {"frames25": (25, dict(obs_frame=1, ee_frame=-2), "RtTableF<5>"),
                          "frames40": (40, dict(obs_frame=1, ee_frame=-2), "trig=1"),
                          "direct64": (64, dict(direct_trig=True), "trig=1"),
                          "lds": (25, dict(dh_in_lds=True), "")}[form]
    p, _ = there_and_back(m, 65536, "rtfrac" if form != "direct64" else "dh7", population, substeps=substeps,
                          test="staged_form_" + form, **kw)
    assert want in p.eng.step_kernel_name(), p.eng.step_kernel_name()


@pytest.mark.parametrize("table_name", ["ref", "rtfrac"])
def test_env_step_on_single_envs_of_a_batch(m, table_name):
    """mt_env_step launches the step kernel on one env: the first envs of the edge list and a few wild ones, one at a
    time, each against the oracle's row."""
    n = 8192
    table, radius = tables(m)[table_name]
    dof = len(table)
    prev, action, rows = sp.edges(0x57A6ED + dof, n, dof, 25)
    p = Pair(m, n, table, radius)
    p.pose(prev)
    p.oracle_step(action)
    chosen = np.unique(np.concatenate([np.arange(0, rows, 7), np.arange(rows, n, 97)]))
    worst = 0.0
    for i in chosen:
        obs, rew, done = p.eng.env_step(int(i), action[i])
        assert obs.shape == (3 * K,)
    zerr = np.abs(p.eng.zmin() - p.ora.zmin)[chosen]
    eerr = np.abs(p.eng.ee() - p.ora.joints_coordinates[:, -1])[chosen]
    print(f"env_step {table_name}: zmin {zerr.max():.3e}  ee {eerr.max():.3e}  over {len(chosen)} envs")
    assert zerr.max() <= POS_TOL and eerr.max() <= POS_TOL, (zerr.max(), eerr.max())
    clear = (np.abs(p.ora.zmin) > GUARD)[chosen] & (np.where(p.pre_alive, p.ora.pickup_margin, np.inf).min(axis=1) > GUARD)[chosen]
    np.testing.assert_array_equal(p.eng.reward()[chosen][clear], p.ref[1][chosen][clear])
    np.testing.assert_array_equal(p.eng.goals()[chosen].view(np.uint32), action[chosen].view(np.uint32))
    untouched = np.setdiff1d(np.arange(n), chosen)
    np.testing.assert_array_equal(p.eng.goals()[untouched].view(np.uint32), prev[untouched].view(np.uint32))
    assert p.eng.bad_action_count() == 0
    record(test="staged_env_step", table=table_name, population="edges", A=32768, kernel=p.eng.step_kernel_name(),
           max_err_zmin=float(zerr.max()), max_err_ee=float(eerr.max()))


# ---- the sub-step trace --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("population", ["wild32768", "local", "edges"])
@pytest.mark.parametrize("table_name", ["ref", "rtfrac"])
def test_substep_trace_against_linspace(m, table_name, population):
    """MT_FLAG_TRACE (the end effector at every sub-step pose of a batch step) and mt_route_trace (joints_coordinates at
    every sub-step pose of given routes): every pose against np.linspace + batch_joints_coordinates in fp64."""
    from oracle import manytor_oracle as mo
    n, S = 8192, 25
    table, radius = tables(m)[table_name]
    dof = len(table)
    prev, action = sp.make(population, 0x7ACE + dof, n, dof, S)
    route = np.linspace(prev.astype(np.float64), action.astype(np.float64), S)             # (S, n, dof)
    want = np.stack([mo.batch_joints_coordinates(route[k], np.asarray(table)) for k in range(S)], axis=1)   # (n, S, dof, 3)
    eng = m.StepEngine(n, K, dh_table=table, radius=radius, trace=True)
    eng.reset_random(3, 0)
    eng.set(m.lib.F_GOALS, prev)
    eng.step(action)
    err_t = np.abs(eng.trace() - want[:, :, -1])
    err_r = np.abs(m.route_trace(prev, action, dh_table=table, substeps=S) - want)
    print(f"trace {table_name} {population}: MT_FLAG_TRACE {err_t.max():.3e}  mt_route_trace {err_r.max():.3e}")
    record(test="staged_trace", table=table_name, population=population, A=amplitude(population),
           max_err_trace=float(err_t.max()), max_err_route_trace=float(err_r.max()))
    assert err_t.max() <= POS_TOL, err_t.max()
    assert err_r.max() <= POS_TOL, err_r.max()


# ---- sampled steps that START from a large pose -----------------------------------------------------------------------
def follower_pair(m, n, table_name, population, seed):
    table, radius = tables(m)[table_name]
    prev, _ = sp.make(population, 0xF011 + len(table), n, len(table))
    p = Pair(m, n, table, radius, seed=seed)
    p.pose(prev)
    return p


def oracle_follows(p, seed, steps):
    """The oracle takes `steps` sampled steps; returns the envs that stayed outside the guard band throughout."""
    from oracle import philox_ref as px
    ids = np.arange(p.n, dtype=np.uint64)
    clean = np.ones(p.n, dtype=bool)
    for t in range(steps):
        act = px.sample_actions(seed, ids, t, p.ora.dof)
        p.oracle_step(act)
        pm = np.where(p.pre_alive, p.ora.pickup_margin, np.inf).min(axis=1)
        clean &= ~((np.abs(p.ora.zmin) < GUARD) | (pm < GUARD))
    return act, clean


def compare_follower(p, act, clean, what, **rec):
    eng, ora = p.eng, p.ora
    np.testing.assert_array_equal(eng.goals(), act)
    zerr = np.abs(eng.zmin() - ora.zmin)
    eerr = np.abs(eng.ee() - ora.joints_coordinates[:, -1]).max(axis=1)
    print(f"{what}: zmin {zerr.max():.3e}  ee {eerr.max():.3e}  clean {clean.mean():.4f}")
    record(kernel=eng.step_kernel_name(), max_err_zmin=float(zerr.max()), max_err_ee=float(eerr.max()), **rec)
    assert zerr.max() <= POS_TOL and eerr.max() <= POS_TOL, (what, zerr.max(), eerr.max())
    assert clean.mean() > 0.97, clean.mean()
    c = clean
    assert_obs_close(eng.obs()[c], p.ref[0][c], ora.joints_coordinates[c, -2], ora.points[c], p.pre_alive[c])
    np.testing.assert_array_equal(eng.reward()[c], p.ref[1][c])
    np.testing.assert_array_equal(eng.alives()[c], ora.alives[c])
    np.testing.assert_array_equal(eng.total_reward()[c], ora.total_reward[c].astype(np.float32))


@pytest.mark.parametrize("population", ["wild32768", "local"])
@pytest.mark.parametrize("table_name", ["ref", "dh7", "rt5"])
@pytest.mark.parametrize("form", ["step_random", "rollout5", "fused3_1lane", "fused3_2lanes", "fused3_4lanes", "graph_replay"])
def test_sampled_steps_from_a_large_pose(m, monkeypatch, form, table_name, population):
    """A sampled action is a whole degree in [-180, 180), but the pose it starts from is whatever was staged or set before:
    mt_step_random, mt_rollout (multi-step kernels: the PoseCache serves from the second step on), mt_rollout_fused with
    1, 2 and 4 lanes per env, and the launch-per-step rollout replayed from its HIP graph."""
    seed = 0xF0110
    n, steps = {"step_random": (262144, 1), "rollout5": (262144, 5), "fused3_1lane": (262144, 3), "fused3_2lanes": (65536, 3),
                "fused3_4lanes": (16384, 3), "graph_replay": (65536, 2)}[form]
    if form == "graph_replay":
        monkeypatch.setenv("MT_ROLLOUT_K", "1")
    p = follower_pair(m, n, table_name, population, seed)
    prev = p.eng.goals()
    act, clean = oracle_follows(p, seed, steps)
    rec = dict(test="staged_follower_" + form, table=table_name, population=population, A=32768)
    if form == "step_random":
        p.eng.step_random(seed, 0)
    elif form == "rollout5":
        assert p.eng.dispatch()["rollout"]["form"] == "multi_step"
        p.eng.rollout(steps, seed, 0)
    elif form == "graph_replay":
        assert p.eng.dispatch()["rollout"]["form"] == "graph_replay"
        want_state = p.eng.get_state()
        p.eng.rollout(steps, seed, 0)                    # captures
        first = {f: p.eng.get(getattr(m.lib, f)) for f in ("F_ZMIN", "F_EE", "F_OBS", "F_REWARD", "F_GOALS")}
        p.eng.set_state(want_state)
        p.eng.set(m.lib.F_GOALS, prev)
        p.eng.rollout(steps, seed, 0)                    # replays
        for f, v in first.items():
            np.testing.assert_array_equal(p.eng.get(getattr(m.lib, f)), v, err_msg=f)
    else:
        lanes = int(form[len("fused3_")])
        assert p.eng.dispatch()["fused"]["lanes_per_env"] == lanes, p.eng.dispatch()["fused"]
        p.eng.rollout_fused(steps, seed, 0)
    compare_follower(p, act, clean, f"{form} {table_name} {population}", **rec)


# ---- the boundary of acceptance ------------------------------------------------------------------------------------------
FIELDS = ("F_GOALS", "F_OBS", "F_REWARD", "F_DONE", "F_ALIVE", "F_EE", "F_TOTAL_REWARD", "F_POINTS", "F_DONE_BITS")


def twin_engines(m, n=512):
    a, b = m.StepEngine(n, K), m.StepEngine(n, K)
    first = np.random.RandomState(5).uniform(-170, 170, size=(n, 4)).astype(np.float32)
    for e in (a, b):
        e.reset_random(9, 0)
        e.step(first)
    return a, b, first


def assert_twins(m, a, b):
    for f in FIELDS:
        np.testing.assert_array_equal(a.get(getattr(m.lib, f)).view(np.uint8), b.get(getattr(m.lib, f)).view(np.uint8), err_msg=f)


def test_the_limit_itself_is_accepted_by_every_door(m):
    """+-32 768.0 through mt_set(F_GOALS), mt_step, mt_env_step and mt_step_host: taken, not counted, and the pose it
    leaves is the oracle's."""
    from oracle import c_oracle
    n = 512
    a, _, first = twin_engines(m, n)
    ora = c_oracle.COracle(n, K, threads=4)
    ora.reset(a.points().astype(np.float64))
    lim = np.where(np.arange(n * 4).reshape(n, 4) % 3 == 0, sp.LIMIT, -sp.LIMIT).astype(np.float32)
    a.set(m.lib.F_GOALS, lim)
    np.testing.assert_array_equal(a.goals(), lim)
    ora.goals[:] = lim
    act = np.random.RandomState(6).uniform(-170, 170, size=(n, 4)).astype(np.float32)
    act[::2] = -lim[::2]
    a.step(act)
    ora.step(act.astype(np.float64))
    np.testing.assert_array_equal(a.goals(), act)
    assert np.abs(a.ee() - ora.joints_coordinates[:, -1]).max() <= POS_TOL
    obs, rew, done = a.env_step(7, lim[7])
    ora_one = ora.goals.copy()
    ora_one[7] = lim[7]
    np.testing.assert_array_equal(a.goals()[7], lim[7])
    obs, rew, done = a.step_host(lim)
    ora.goals[:] = ora_one
    ora.step(lim.astype(np.float64))
    np.testing.assert_array_equal(a.goals(), lim)
    assert np.abs(a.ee() - ora.joints_coordinates[:, -1]).max() <= POS_TOL
    assert a.bad_action_count() == 0


def test_the_first_float_beyond_the_limit_is_refused_or_held_and_counted(m):
    """nextafter(32768, inf): mt_set refuses the array (nothing stored); mt_step, mt_env_step and mt_step_host hold the pose of
    that env and count it -- every field bit for bit what a twin handle shows that was handed the held pose instead."""
    n = 512
    a, b, first = twin_engines(m, n)
    over = first.copy()
    over[11, 2] = sp.ABOVE
    over[300, 0] = -sp.ABOVE
    with pytest.raises((ValueError, RuntimeError)):
        a.set(m.lib.F_GOALS, over)
    assert_twins(m, a, b)
    act = np.random.RandomState(7).uniform(-170, 170, size=(n, 4)).astype(np.float32)
    bad, hold = act.copy(), act.copy()
    bad[11, 2], bad[300, 0] = sp.ABOVE, -sp.ABOVE
    hold[11], hold[300] = first[11], first[300]
    a.step(bad)
    b.step(hold)
    assert a.bad_action_count() == 2 and b.bad_action_count() == 0
    assert_twins(m, a, b)
    one = act[5].copy()
    one[3] = sp.ABOVE
    a.env_step(5, one)
    b.env_step(5, hold[5])
    assert a.bad_action_count() == 3
    assert_twins(m, a, b)
    act2 = np.random.RandomState(8).uniform(-170, 170, size=(n, 4)).astype(np.float32)
    bad2, hold2 = act2.copy(), act2.copy()
    bad2[99, 1] = -sp.ABOVE
    hold2[99] = a.goals()[99]
    oa = a.step_host(bad2)
    ob = b.step_host(hold2)
    assert a.bad_action_count() == 4
    for x, y in zip(oa, ob):
        np.testing.assert_array_equal(x, y)
    assert_twins(m, a, b)
