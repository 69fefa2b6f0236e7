"""mt_rollout_tape / StepEngine.rollout_actions / Multienv.step_sequence: T steps with the CALLER's actions in one launch.

Held to two references:
  * the launch-per-step path it replaces -- set_actions(tape[t]); step(); [reset_done(seed)] -- bit for bit (state, last
    step's outputs, per-step logs), for tapes inside +-180 degrees;
  * the fp64 C restatement of the reference (oracle/manytor_oracle.c), every env, stepped T times on the host with the
    same tape, re-arming finished envs the way the kernel does.  An env is compared while the oracle's own decision
    margins stayed above GUARD at every step so far (tests/test_gpu_fused_oracle.py: same rule); every case must
    compare at least 95 % of its envs.

Reference semantics: manytor.py:255-260 per step, :175-213 for the action, test_multi.py:17-34 for the loop.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import staged_populations as sp
from parity_util import GUARD, POS_TOL, assert_obs_close

pytestmark = pytest.mark.gpu

SEED = 0x7A9E
RING = 8
MIN_CLEAN = 0.95


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def _table(m, name):
    if name == "ref":
        return m.REF_DH_TABLE, 51.3
    if name == "dh7":
        return m.DH7_TABLE, 92.6
    if name.startswith("dof"):               # "dof3": a runtime table of that many joints, test_gpu_parity.py's recipe
        dof = int(name[3:])
        rng = np.random.RandomState(dof)
        return np.column_stack([rng.uniform(0, 10, dof), rng.choice([-np.pi / 2, 0, np.pi / 2, 0.4], dof),
                                rng.uniform(2, 15, dof), rng.choice([0, -np.pi / 2, 0.25], dof)]), 40.0
    return sp.fractional_offset_table()      # "rt5": runtime table, theta offsets that are no whole degrees


@functools.lru_cache(maxsize=None)
def narrow_tape(T, n, D):
    t = np.random.RandomState(SEED + T + n).uniform(-180, 180, (T, n, D)).astype(np.float32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def turns_tape(T, n, D):
    rng = np.random.RandomState(SEED + T + n)
    small = rng.uniform(-60, 60, (T, n, D))
    turns = rng.randint(-90, 91, (1, n, D))
    t = (small + 360.0 * turns).astype(np.float32)
    t.setflags(write=False)
    return t


def make_engine(m, table_name, n, k, tol, **kw):
    table, radius = _table(m, table_name)
    eng = m.StepEngine(n, k, dh_table=table, radius=radius, pickup_tol=tol, return_ring=RING, debug_zmin=True, **kw)
    return eng


STATE = ("F_GOALS", "F_POINTS", "F_ALIVE", "F_TOTAL_REWARD", "F_EPISODES", "F_LAST_RETURN", "F_RETURN_RING")
OUTPUTS = ("F_OBS", "F_REWARD", "F_DONE", "F_DONE_BITS", "F_EE", "F_ZMIN")
EVERYTHING = ("F_ACTIONS",) + STATE + OUTPUTS


def snapshot(m, eng, fields):
    return {f: eng.get(getattr(m.lib, f)) for f in fields}


def assert_same(got, want, what=""):
    assert got.keys() == want.keys()
    for f in want:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what} {f}")


def run_per_step(m, eng, tape, auto_reset):
    """The path the tape call replaces: one staging + one step launch (+ one re-arm launch) per step.  Returns the state
    after the last step, the last step's outputs as they were BEFORE its re-arm launch, and the per-step records."""
    T = tape.shape[0]
    rew, done = [], []
    outs = None
    for t in range(T):
        eng.set_actions(tape[t])
        eng.step()
        rew.append(eng.reward())
        done.append(eng.get(m.lib.F_DONE))
        if t == T - 1:
            outs = snapshot(m, eng, OUTPUTS)
        if auto_reset:
            eng.reset_done(SEED)
    return snapshot(m, eng, STATE), outs, np.stack(rew), np.stack(done)


# ---- 1. bit identity with the launch-per-step path ---------------------------------------------------------------
# `rearmed`: with auto_reset, the number of envs that must have finished at least once.  The fp64 oracle alone, run on the
# host for exactly these inputs, finishes 136 / 32 855 / 61 / 97 envs in the four auto-reset cases; the floors are about
# half of that (an env inside the guard band may finish on one side only).  ref at 300 007 envs and tol 8 finishes none
# in 6 steps, so that size runs without auto_reset only.
@pytest.mark.parametrize("table_name,n,k,T,tol,auto_reset,rearmed", [
    ("ref", 3001, 7, 12, 8.0, False, 0),
    ("ref", 3001, 7, 12, 20.0, True, 60),
    ("dh7", 70001, 3, 8, 45.0, False, 0),
    ("dh7", 70001, 3, 8, 45.0, True, 16000),
    ("rt5", 9001, 3, 8, 8.0, False, 0),
    ("rt5", 9001, 3, 8, 8.0, True, 30),
    ("ref", 777, 32, 10, 30.0, False, 0),    # K = 32: the 96 KB LDS tile
    ("ref", 777, 32, 10, 30.0, True, 50),
    ("ref", 300007, 7, 6, 8.0, False, 0),    # a two-chain handle on the per-step side
])
def test_tape_is_bit_identical_to_the_launch_per_step_path(m, table_name, n, k, T, tol, auto_reset, rearmed):
    a = make_engine(m, table_name, n, k, tol)
    b = make_engine(m, table_name, n, k, tol)
    tape = narrow_tape(T, n, a.dof)
    for e in (a, b):
        e.reset_random(SEED, 0)
    state_a, outs_a, rew_a, done_a = run_per_step(m, a, tape, auto_reset)
    res = b.rollout_actions(tape, auto_reset=auto_reset, seed=SEED, log=True, returns=True)
    b.sync()
    assert_same(snapshot(m, b, STATE), state_a, "state")
    # the last step's outputs: an env re-armed in the last step keeps done == 2, everything else as the step left it
    want = dict(outs_a)
    want["F_DONE"] = np.where(outs_a["F_DONE"] != 0, 2 if auto_reset else 1, 0).astype(np.uint8)
    assert_same(snapshot(m, b, OUTPUTS), want, "outputs")
    np.testing.assert_array_equal(b.actions(), tape[-1])          # what set_actions(tape[T - 1]) left on the other side
    rew_b, done_b = res["reward"].cpu().numpy(), res["done"].cpu().numpy()
    assert rew_b.dtype == np.int8 and done_b.dtype == np.uint8 and rew_b.shape == (T, n) and done_b.shape == (T, n)
    np.testing.assert_array_equal(rew_b, rew_a)
    np.testing.assert_array_equal(done_b, (done_a != 0).astype(np.uint8))
    np.testing.assert_array_equal(res["returns"].cpu().numpy(), rew_a.sum(axis=0).astype(np.float32))
    assert b.bad_action_count() == 0 and a.bad_action_count() == 0
    if auto_reset:
        assert (b.finished() > 0).sum() > rearmed, "the re-arm path was not exercised"
    a.close()
    b.close()


# ---- 2. against the fp64 oracle, every env -----------------------------------------------------------------------
def unusable(row):
    """(n,) bool: the env's action of this step has a component the kernels refuse (kernels.h: unusable_angle)."""
    return (~np.isfinite(row) | (np.abs(row) > np.float32(32768.0))).any(axis=1)


def run_tape_against_oracle(m, table_name, n, k, T, tol, auto_reset, tape, substeps=25, terminate_on_ground=False,
                            specialize=True, episode0=0, start_pose=None):
    """One committing rollout_actions call on the GPU vs T oracle steps on the host; returns what the callers assert on.
    episode0: the full reset in front of the call is reset_random(SEED, episode0).  start_pose: fp32 (n, D) joint angles
    written with eng.set(MT_F_GOALS) behind that reset.  terminate_on_ground: the oracle has no such flag; the episode of an
    env that touched the ground (reward == -1) ends here, ahead of the re-arm and of the comparison of the done log."""
    from oracle import c_oracle
    from oracle import philox_ref as px
    table, radius = _table(m, table_name)
    eng = make_engine(m, table_name, n, k, tol, substeps=substeps, terminate_on_ground=terminate_on_ground, specialize=specialize)
    ora = c_oracle.COracle(n, k, table=np.asarray(table), substeps=substeps, radius=radius, pickup_tol=tol, threads=16)
    ids = np.arange(n, dtype=np.uint64)
    eng.reset_random(SEED, episode0)
    ora.reset(eng.points().astype(np.float64))
    if start_pose is not None:
        eng.set(m.lib.F_GOALS, start_pose)
        ora.goals[:] = start_pose.astype(np.float64)
    res = eng.rollout_actions(tape, auto_reset=auto_reset, seed=SEED, log=True, returns=True)      # ONE launch
    eng.sync()
    rew_log, done_log = res["reward"].cpu().numpy(), res["done"].cpu().numpy()

    clean = np.ones(n, dtype=bool)
    episodes = np.full(n, episode0, dtype=np.int64)
    last_ret = np.zeros(n)
    ring = np.zeros((n, RING))
    written = np.zeros((n, RING), dtype=bool)                      # slots an env has actually written
    ret = np.zeros(n)
    held = 0
    last = None
    for t in range(T):
        bad = unusable(tape[t])
        held += int(bad.sum())
        act = np.where(bad[:, None], ora.goals, tape[t].astype(np.float64))     # an unusable action: the pose is held
        pre_alive = ora.alives.copy()
        obs_ref, rew_ref, done_ref = ora.step(act)
        if terminate_on_ground:
            done_ref = done_ref | (rew_ref == -1)
        pm = np.where(pre_alive, ora.pickup_margin, np.inf).min(axis=1)
        clean &= ~((ora.ground_margin < GUARD) | (pm < GUARD))
        ret += rew_ref
        # the logs of this step, for the envs that are clean up to and including it
        np.testing.assert_array_equal(rew_log[t][clean], rew_ref[clean], err_msg=f"reward log, step {t}")
        np.testing.assert_array_equal(done_log[t][clean], done_ref[clean].astype(np.uint8), err_msg=f"done log, step {t}")
        if t == T - 1:
            last = dict(obs=obs_ref, rew=rew_ref, done=done_ref, jc=ora.joints_coordinates.copy(), pre_alive=pre_alive,
                        points=ora.points.copy(), zmin=ora.zmin.copy())
        if auto_reset and done_ref.any():                          # what the kernel does in the step an env finishes
            idx = np.flatnonzero(done_ref)
            slot = (episodes[idx] - episode0) % RING               # include/manytor_hip.h: MT_F_RETURN_RING
            ring[idx, slot] = ora.total_reward[idx]
            written[idx, slot] = True
            last_ret[idx] = ora.total_reward[idx]
            episodes[idx] += 1
            ora.goals[idx] = 0.0
            ora.total_reward[idx] = 0.0
            ora.alive_u8[idx] = 1
            ora.points[idx] = px.sample_targets(SEED, ids[idx], episodes[idx], k, radius).astype(np.float64)

    c = clean
    finished = episodes - episode0
    print(f"[tape-vs-oracle] {table_name} n={n} K={k} T={T} tol={tol} auto_reset={auto_reset} S={substeps} "
          f"terminate={terminate_on_ground} specialize={specialize} episode0={episode0} "
          f"start_pose={'no' if start_pose is None else 'yes'}: clean share {c.mean():.4f}, "
          f"re-arms {int(finished.sum())}, max episodes {int(finished.max())}, held env-steps {held}")
    assert c.mean() >= MIN_CLEAN, c.mean()
    np.testing.assert_array_equal(eng.goals()[c], ora.goals[c].astype(np.float32))
    np.testing.assert_array_equal(eng.alives()[c], ora.alives[c])
    np.testing.assert_array_equal(eng.total_reward()[c], ora.total_reward[c].astype(np.float32))
    np.testing.assert_array_equal(eng.points()[c], ora.points[c].astype(np.float32))
    np.testing.assert_array_equal(eng.episodes()[c], episodes[c])
    np.testing.assert_array_equal(res["returns"].cpu().numpy()[c], ret[c].astype(np.float32))
    if auto_reset:
        fin = c & (finished > 0)
        np.testing.assert_array_equal(eng.last_return()[fin], last_ret[fin].astype(np.float32))
        sel = written & c[:, None]
        np.testing.assert_array_equal(eng.return_ring()[sel], ring[sel].astype(np.float32))
    np.testing.assert_array_equal(eng.reward()[c], last["rew"][c])
    done_raw = eng.get(m.lib.F_DONE)
    np.testing.assert_array_equal(done_raw[c] != 0, last["done"][c])
    assert set(np.unique(done_raw)) <= ({0, 2} if auto_reset else {0, 1})
    assert np.abs(eng.ee() - last["jc"][:, -1]).max() <= POS_TOL    # continuous: every env, guard band or not
    assert_obs_close(eng.obs()[c], last["obs"][c], last["jc"][c, -2], last["points"][c], last["pre_alive"][c])
    assert np.abs(eng.zmin() - last["zmin"])[c].max() <= GUARD
    assert eng.bad_action_count() == held
    return dict(eng=eng, clean=c, episodes=finished, finished=int((finished > 0).sum()), max_episodes=int(finished.max()),
                rearms=int(finished.sum()), ring_written=int((written & c[:, None]).sum()))


@pytest.mark.parametrize("table_name,n,k,T,tol,auto_reset,kind", [
    ("ref", 3001, 7, 12, 8.0, False, "narrow"),
    ("ref", 3001, 3, 24, 20.0, True, "narrow"),
    ("dh7", 70001, 7, 8, 8.0, False, "narrow"),
    ("dh7", 70001, 3, 16, 45.0, True, "narrow"),
    ("ref", 777, 32, 10, 30.0, True, "narrow"),
    ("ref", 300007, 7, 6, 8.0, False, "narrow"),
    ("ref", 3001, 7, 8, 8.0, False, "turns"),        # angles up to +-31 344 degrees: the wide routes, per wave
    ("dh7", 70001, 3, 8, 45.0, True, "turns"),
])
def test_tape_every_env_against_the_c_oracle(m, table_name, n, k, T, tol, auto_reset, kind):
    D = len(_table(m, table_name)[0])
    tape = (narrow_tape if kind == "narrow" else turns_tape)(T, n, D)
    if kind == "turns":
        assert np.abs(tape).max() > 30000
    stats = run_tape_against_oracle(m, table_name, n, k, T, tol, auto_reset, tape)
    if auto_reset:
        assert stats["finished"] > 50, stats                       # the re-arm path was really exercised
        if table_name == "dh7" and kind == "narrow":
            assert stats["max_episodes"] >= 2, stats
    stats["eng"].close()


# ---- 3. dry run --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table_name,n,k,T,tol,kind", [
    ("ref", 3001, 7, 12, 8.0, "narrow"),
    ("dh7", 70001, 3, 8, 45.0, "turns"),
])
def test_dry_run_changes_nothing_resident_and_predicts_the_committing_call(m, table_name, n, k, T, tol, kind):
    eng = make_engine(m, table_name, n, k, tol)
    tape = (narrow_tape if kind == "narrow" else turns_tape)(T, n, eng.dof)
    eng.reset_random(SEED, 0)
    eng.rollout_actions(tape[:2])                                  # a state with history: outputs, dead targets, returns
    eng.set_actions(tape[1] + np.float32(0.5))                     # ... and an action row that no call below would write
    planted = tape.copy()
    planted[1, 7, 0] = np.nan                                      # a dry run must not count either
    before = snapshot(m, eng, EVERYTHING)
    bad_before = eng.bad_action_count()
    version = eng.version
    dry = eng.rollout_actions(planted, dry_run=True, log=True, returns=True)
    eng.sync()
    assert_same(snapshot(m, eng, EVERYTHING), before, "after the dry run")
    assert eng.bad_action_count() == bad_before and eng.version == version
    real = eng.rollout_actions(planted, log=True, returns=True)
    eng.sync()
    assert eng.version == version + 1 and eng.bad_action_count() == bad_before + 1
    for key in ("reward", "done", "returns"):
        np.testing.assert_array_equal(dry[key].cpu().numpy(), real[key].cpu().numpy(), err_msg=key)
    assert np.abs(real["reward"].cpu().numpy()).sum() > 0          # (something happened in those T steps)
    with pytest.raises(ValueError):
        eng.rollout_actions(tape, dry_run=True, auto_reset=True)
    eng.close()


# ---- 4. screening ------------------------------------------------------------------------------------------------
def test_unusable_actions_hold_the_pose_and_are_counted(m):
    n, k, T, tol = 3001, 7, 12, 8.0
    tape = narrow_tape(T, n, 4).copy()
    tape[2, 5, 1] = np.nan
    tape[2, 5, 3] = np.nan              # the same (step, env) pair: counted once
    tape[0, 100, 0] = np.inf            # in the very first step: the held pose is the reset's zero pose
    tape[4, 1234, 2] = -np.inf
    tape[5, 2999, 3] = sp.ABOVE         # the first float that is refused
    tape[T - 1, 64, 0] = np.nan         # in the last step: the final pose is the one of step T - 2
    tape[3, 700, 2] = sp.BELOW          # accepted: the largest float under the limit
    tape[7, 65, 0] = -sp.LIMIT          # accepted: the limit itself (env 65 shares a wave with the held env 64)
    tape[T - 1, 900, 1] = sp.LIMIT
    tape[T - 1, 901, 3] = -sp.BELOW
    n_pairs = 5
    stats = run_tape_against_oracle(m, "ref", n, k, T, tol, False, tape)       # mirrors the hold, asserts the count
    eng = stats["eng"]
    assert eng.bad_action_count() == n_pairs
    goals = eng.goals()
    np.testing.assert_array_equal(goals[64], tape[T - 2, 64])                  # held in the last step
    assert goals[900, 1] == sp.LIMIT and goals[901, 3] == -sp.BELOW            # accepted as they are
    for f, v in snapshot(m, eng, EVERYTHING).items():
        if v.dtype.kind == "f" and f != "F_ACTIONS":                           # (MT_F_ACTIONS is the raw staged row)
            assert np.isfinite(v).all(), f
    # the same through a single-step call: pose before == pose after, for exactly the refused envs
    before = eng.goals()
    row = narrow_tape(1, n, 4).copy()
    refused = np.array([0, 63, 64, 255, 256, 1500, 3000])
    row[0, refused[0], 0] = np.nan
    row[0, refused[1], 1] = np.inf
    row[0, refused[2], 2] = -np.inf
    row[0, refused[3], 3] = sp.ABOVE
    row[0, refused[4], 0] = -sp.ABOVE
    row[0, refused[5]] = np.nan
    row[0, refused[6], 3] = np.float32(1e30)
    row[0, 1, 0] = sp.BELOW
    row[0, 2, 0] = sp.LIMIT
    log = eng.rollout_actions(row, log=True)
    eng.sync()
    after = eng.goals()
    ok = np.ones(n, dtype=bool)
    ok[refused] = False
    np.testing.assert_array_equal(after[refused], before[refused])
    np.testing.assert_array_equal(after[ok], row[0][ok])
    assert eng.bad_action_count() == n_pairs + len(refused)
    assert set(np.unique(log["reward"].cpu().numpy())) <= {-1, 0, 1}
    assert np.isfinite(eng.ee()).all() and np.isfinite(eng.obs()).all() and np.isfinite(eng.zmin()).all()
    eng.close()


# ---- 5. stream order on a caller's stream ------------------------------------------------------------------------
def test_tape_call_is_ordered_with_torch_ops_on_the_callers_stream(m):
    import torch
    n, k, T, tol = 3001, 7, 12, 8.0
    tape = np.ascontiguousarray(narrow_tape(T, n, 4).transpose(0, 2, 1))       # (T, D, N)
    own = make_engine(m, "ref", n, k, tol)
    own.reset_random(SEED, 0)
    want = own.rollout_actions(tape, layout="soa", log=True, returns=True)
    own.sync()
    want_sum = want["reward"].to(torch.int32).sum(dim=0).cpu().numpy()

    eng = make_engine(m, "ref", n, k, tol)
    eng.use_torch_stream()
    eng.reset_random(SEED, 0)
    dev = torch.device("cuda", eng.device)
    src = torch.from_numpy(tape).to(dev)
    buf = torch.zeros_like(src)
    ballast = torch.ones((2048, 2048), device=dev)
    torch.cuda.synchronize(dev)
    for _ in range(8):                                             # keeps the stream busy ahead of the tape's writer
        ballast = ballast @ ballast * 1e-4
    buf.copy_(src)                                                 # the torch op that writes the tape ...
    res = eng.rollout_actions(buf, layout="soa", log=True, returns=True)       # ... read in place, no host sync ...
    got_sum = res["reward"].to(torch.int32).sum(dim=0)             # ... and a torch reduction of the log right behind
    buf.zero_()                                                    # (a later write must not reach the call either)
    torch.cuda.synchronize(dev)
    np.testing.assert_array_equal(got_sum.cpu().numpy(), want_sum)
    np.testing.assert_array_equal(res["returns"].cpu().numpy(), want["returns"].cpu().numpy())
    assert_same(snapshot(m, eng, STATE + OUTPUTS), snapshot(m, own, STATE + OUTPUTS), "caller's stream vs own stream")
    assert np.abs(want_sum).sum() > 0
    eng.close()
    own.close()


# ---- 6. strided tape and log pitch -------------------------------------------------------------------------------
def test_tape_pitch_and_log_pitch_through_the_c_entry_point(m):
    import torch
    n, k, T, tol, D = 3001, 7, 12, 8.0, 4
    ld, log_ld = n + 37, n + 5
    tape = np.ascontiguousarray(narrow_tape(T, n, D).transpose(0, 2, 1))       # (T, D, N)
    dense = make_engine(m, "ref", n, k, tol)
    dense.reset_random(SEED, 0)
    want = dense.rollout_actions(tape, layout="soa", log=True, returns=True)
    dense.sync()

    eng = make_engine(m, "ref", n, k, tol)
    eng.reset_random(SEED, 0)
    dev = torch.device("cuda", eng.device)
    padded = torch.full((T * D, ld), float("nan"), dtype=torch.float32, device=dev)     # pad columns are never read
    padded[:, :n] = torch.from_numpy(tape.reshape(T * D, n)).to(dev)
    rew = torch.full((T, log_ld), 0x55, dtype=torch.int8, device=dev)
    done = torch.full((T, log_ld), 0xAA, dtype=torch.uint8, device=dev)
    ret = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    arg = m.lib.MtTape()
    arg.struct_size, arg.n_steps, arg.actions, arg.ld = C.sizeof(m.lib.MtTape), T, padded.data_ptr(), ld
    arg.reward_log, arg.done_log, arg.log_ld, arg.return_out = rew.data_ptr(), done.data_ptr(), log_ld, ret.data_ptr()
    arg.seed, arg.flags = SEED, 0
    assert eng._lib.mt_rollout_tape(eng._h, C.byref(arg)) == m.lib.MT_OK, eng._lib.mt_last_error(eng._h)
    eng.sync()
    rew, done = rew.cpu().numpy(), done.cpu().numpy()
    np.testing.assert_array_equal(rew[:, :n], want["reward"].cpu().numpy())
    np.testing.assert_array_equal(done[:, :n], want["done"].cpu().numpy())
    assert (rew[:, n:] == 0x55).all() and (done[:, n:] == 0xAA).all()          # the pad columns are untouched
    np.testing.assert_array_equal(ret.cpu().numpy(), want["returns"].cpu().numpy())
    assert_same(snapshot(m, eng, STATE + OUTPUTS), snapshot(m, dense, STATE + OUTPUTS), "pitched vs dense")
    # the same pitch through the Python front end: a (T, D, N) view of the padded rows goes in zero-copy
    view = padded.view(T, D, ld)[:, :, :n]
    assert eng._tape_tensor(view, "soa")[0].data_ptr() == padded.data_ptr() and eng._tape_tensor(view, "soa")[1] == ld
    strided = torch.zeros((T, D, 2 * n), dtype=torch.float32, device=dev)[:, :, ::2]     # env stride 2: made contiguous
    made, made_ld = eng._tape_tensor(strided, "soa")
    assert made_ld == n and made.is_contiguous() and made.data_ptr() != strided.data_ptr()
    eng.close()
    dense.close()


# ---- 7. errors ---------------------------------------------------------------------------------------------------
def test_error_returns_and_dispatch_entry(m):
    import torch
    L = m.lib
    n, T, D = 3001, 3, 4
    eng = make_engine(m, "ref", n, 7, 8.0)
    dev = torch.device("cuda", eng.device)
    tape = torch.zeros((T * D, n), dtype=torch.float32, device=dev)
    logs = torch.zeros((T, n), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)

    def call(engine=eng, **over):
        arg = L.MtTape()
        arg.struct_size, arg.n_steps, arg.actions, arg.ld, arg.log_ld = C.sizeof(L.MtTape), T, tape.data_ptr(), n, n
        for key, v in over.items():
            setattr(arg, key, v)
        rc = engine._lib.mt_rollout_tape(engine._h, C.byref(arg))
        return rc, engine._lib.mt_last_error(engine._h).decode()

    rc, msg = call()
    assert rc == L.MT_ERR_STATE and "reset" in msg                              # before a reset
    eng.reset_random(SEED, 0)
    assert call(log_ld=0)[0] == L.MT_OK                                         # no log given: the pitch is not looked at
    eng.sync()
    before = snapshot(m, eng, EVERYTHING)
    assert call(actions=None)[0] == L.MT_ERR_INVALID_ARG
    assert call(ld=n - 1)[0] == L.MT_ERR_INVALID_ARG
    assert call(reward_log=logs.data_ptr(), log_ld=n - 1)[0] == L.MT_ERR_INVALID_ARG
    assert call(done_log=logs.data_ptr(), log_ld=0)[0] == L.MT_ERR_INVALID_ARG
    rc, msg = call(struct_size=C.sizeof(L.MtTape) - 8)
    assert rc == L.MT_ERR_INVALID_ARG and "struct_size" in msg
    assert call(reserved=1)[0] == L.MT_ERR_INVALID_ARG
    assert call(n_steps=-1)[0] == L.MT_ERR_INVALID_ARG
    assert call(flags=0x4)[0] == L.MT_ERR_INVALID_ARG
    rc, msg = call(flags=L.TAPE_DRY_RUN | L.TAPE_AUTO_RESET)
    assert rc == L.MT_ERR_INVALID_ARG and "DRY_RUN" in msg
    assert call(n_steps=0, actions=None)[0] == L.MT_OK                          # T = 0: a no-op
    eng.sync()
    assert_same(snapshot(m, eng, EVERYTHING), before, "after the refused calls and T = 0")
    assert eng.rollout_actions(np.zeros((0, n, D), dtype=np.float32)) is None
    with pytest.raises(ValueError):
        eng.rollout_actions(np.zeros((T, n, D + 1), dtype=np.float32))
    with pytest.raises(ValueError):
        eng.rollout_actions(np.zeros((T, n, D), dtype=np.float32), layout="rows")

    hw = make_engine(m, "ref", n, 7, 8.0, hw_trig=True)
    hw.reset_random(SEED, 0)
    rc, msg = call(engine=hw)
    assert rc == L.MT_ERR_UNSUPPORTED and "MT_FLAG_HW_TRIG" in msg
    with pytest.raises(m.ManytorError):
        hw.rollout_actions(np.zeros((T, n, D), dtype=np.float32))
    assert hw.dispatch()["tape"]["usable"] is False
    d = eng.dispatch()["tape"]
    assert d["usable"] is True and d["lanes_per_env"] == 1 and d["chains"] == 1
    hw.close()
    eng.close()


# ---- 8. Multienv.step_sequence ------------------------------------------------------------------------------------
def test_multienv_step_sequence_equals_repeated_step(m):
    T = 6
    a = m.Multienv((3, 2), 7, rng="device", seed=SEED)
    b = m.Multienv((3, 2), 7, rng="device", seed=SEED)
    a.reset()
    b.reset()
    acts = np.random.RandomState(SEED).randint(-180, 180, size=(T, 6, 4))
    as_lists = [[[int(v) for v in row] for row in step] for step in acts]
    steps = [a.step(as_lists[t]) for t in range(T)]
    obs, rewards, dones = b.step_sequence(as_lists)
    assert isinstance(obs, list) and len(obs) == 6 and obs[0].dtype == np.float64
    np.testing.assert_array_equal(np.stack(obs), np.stack(steps[-1][0]))
    assert rewards == [s[1] for s in steps] and dones == [s[2] for s in steps]
    assert all(type(v) is int for row in rewards for v in row) and all(type(v) is bool for row in dones for v in row)
    assert b._step_idx == a._step_idx == T
    np.testing.assert_array_equal(b.engine.goals(), a.engine.goals())
    np.testing.assert_array_equal(b.engine.total_reward(), a.engine.total_reward())
    a.close()
    b.close()


def test_multienv_step_sequence_large_batch_returns_views_and_arrays(m):
    T, n = 4, 5000
    env = m.Multienv((50, 100), 7, rng="device", seed=SEED)
    env.reset()
    obs, rewards, dones = env.step_sequence(narrow_tape(T, n, 4))
    assert isinstance(obs, m.BatchView) and obs.numpy().shape == (n, 21)
    assert isinstance(rewards, np.ndarray) and rewards.shape == (T, n) and rewards.dtype == np.int8
    assert isinstance(dones, np.ndarray) and dones.shape == (T, n) and dones.dtype == bool
    assert env._step_idx == T
    np.testing.assert_array_equal(env.engine.reward(), rewards[-1])
    np.testing.assert_array_equal(env.engine.total_reward(), rewards.sum(axis=0).astype(np.float32))
    env.close()
