"""mt_rollout_tape across the engine's options, the two shipped switches and stream capture.

tests/test_gpu_tape.py runs the tape kernel on default handles.  The kernel accepts every handle the fused rollout accepts
(engine.hip: fusable), so here it runs with MT_FLAG_TERMINATE_ON_GROUND, other sub-step counts (S <= 9: the increment comes
from sincos_deg; S = 26: the last one the recurrence takes), the reference table as a runtime table (specialize=False), the
generic runtime-table form at D = 2, 3, 5, 8, K = 1, batches ragged around a wave, a full reset at an episode base other
than 0 with the return ring wrapping around, a start pose beyond +-180 degrees read from memory, one tape split over two
calls, MT_TAPE_PREFETCH / MT_TAPE_NT (four kernel instantiations nothing else launches), and inside a captured HIP graph.

Two references, as in tests/test_gpu_tape.py: the launch-per-step path on a twin, bit for bit, and the fp64 C oracle for every
env outside the guard band (run_tape_against_oracle, at least MIN_CLEAN of the envs; it prints the clean share of each
case.  The shares below are the oracle's alone for these inputs, measured on the host)."""
import ctypes as C

import numpy as np
import pytest

import staged_populations as sp
from test_gpu_tape import (EVERYTHING, OUTPUTS, RING, SEED, STATE, _table, assert_same, make_engine, narrow_tape, run_per_step,
                           run_tape_against_oracle, snapshot, turns_tape)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def _arm(m, eng, episode0, start_pose):
    eng.reset_random(SEED, episode0)
    if start_pose is not None:
        eng.set(m.lib.F_GOALS, start_pose)


def assert_tape_equals_per_step(m, table_name, n, k, tol, tape, auto_reset, episode0=0, start_pose=None, **options):
    """rollout_actions(tape) on one handle against set_actions(row); step(); [reset_done] on its twin: state, the last step's
    outputs, the staged row, per-step logs, returns and the held-action count, bit for bit.  Returns the tape side's result."""
    a = make_engine(m, table_name, n, k, tol, **options)
    b = make_engine(m, table_name, n, k, tol, **options)
    for e in (a, b):
        _arm(m, e, episode0, start_pose)
    state_a, outs_a, rew_a, done_a = run_per_step(m, a, tape, auto_reset)
    res = b.rollout_actions(tape, auto_reset=auto_reset, seed=SEED, log=True, returns=True)
    b.sync()
    assert_same(snapshot(m, b, STATE), state_a, "state")
    want = dict(outs_a)                  # an env re-armed in the last step keeps done == 2, everything else as the step left it
    want["F_DONE"] = np.where(outs_a["F_DONE"] != 0, 2 if auto_reset else 1, 0).astype(np.uint8)
    assert_same(snapshot(m, b, OUTPUTS), want, "outputs")
    np.testing.assert_array_equal(b.actions(), tape[-1])
    out = {key: v.cpu().numpy() for key, v in res.items()}
    np.testing.assert_array_equal(out["reward"], rew_a)
    np.testing.assert_array_equal(out["done"], (done_a != 0).astype(np.uint8))
    np.testing.assert_array_equal(out["returns"], rew_a.sum(axis=0).astype(np.float32))
    assert a.bad_action_count() == b.bad_action_count()
    out["finished"] = b.finished()
    out["bad"] = b.bad_action_count()
    a.close()
    b.close()
    return out


# ---- B. MT_TAPE_PREFETCH / MT_TAPE_NT ----------------------------------------------------------------------------------------
def planted_tape(T, n, D):
    """narrow_tape with held actions where the prefetch form reorders loads around them: in step 0 (the row loaded ahead of
    the loop), in the last step (no row behind it), and mid-tape next to an accepted neighbour."""
    tape = narrow_tape(T, n, D).copy()
    tape[0, 100, 0] = np.nan
    tape[T - 1, 64, D - 1] = np.nan
    tape[5, 2999, 1] = sp.ABOVE
    tape[5, 2998, 1] = sp.BELOW
    return tape, 3


@pytest.mark.parametrize("switches,table_name", [
    (("MT_TAPE_PREFETCH",), "ref"),
    (("MT_TAPE_PREFETCH",), "dh7"),
    (("MT_TAPE_PREFETCH",), "rt5"),      # no prefetch form for runtime tables: reported off, same bits
    (("MT_TAPE_NT",), "ref"),
    (("MT_TAPE_NT",), "rt5"),
    (("MT_TAPE_PREFETCH", "MT_TAPE_NT"), "ref"),
])
def test_shipped_switches_give_the_same_bits(m, monkeypatch, switches, table_name):
    n, k, T = 3001, 7, 12
    tol = 45.0 if table_name == "dh7" else 20.0       # (the oracle alone re-arms 137 / 1133 / 2007 times: ref / dh7 / rt5)
    for key in switches:
        monkeypatch.setenv(key, "1")
    switched = make_engine(m, table_name, n, k, tol)
    for key in switches:
        monkeypatch.delenv(key)
    plain = make_engine(m, table_name, n, k, tol)
    d, p = switched.dispatch(), plain.dispatch()
    assert d["tape"]["prefetch"] is ("MT_TAPE_PREFETCH" in switches and table_name != "rt5"), d["tape"]
    assert d["tape"]["nt_loads"] is ("MT_TAPE_NT" in switches), d["tape"]
    for key in ("MT_TAPE_PREFETCH", "MT_TAPE_NT"):
        assert (f"{key}=1" in d["overrides"].split(",")) == (key in switches), d["overrides"]
        assert f"{key}=" not in p["overrides"], p["overrides"]
    assert p["tape"]["prefetch"] is False and p["tape"]["nt_loads"] is False
    tape, held = planted_tape(T, n, switched.dof)
    got = []
    for eng in (switched, plain):
        eng.reset_random(SEED, 0)
        res = eng.rollout_actions(tape, auto_reset=True, seed=SEED, log=True, returns=True)
        eng.sync()
        got.append((snapshot(m, eng, EVERYTHING), {key: v.cpu().numpy() for key, v in res.items()}, eng.bad_action_count()))
        eng.close()
    assert_same(got[0][0], got[1][0], "switched vs plain")
    assert_same(got[0][1], got[1][1], "switched vs plain, logs")
    per = assert_tape_equals_per_step(m, table_name, n, k, tol, tape, True)      # (the plain form again, against the steps)
    assert_same({key: per[key] for key in ("reward", "done", "returns")}, got[0][1], "switched vs per step, logs")
    assert got[0][2] == got[1][2] == per["bad"] == held
    assert (per["finished"] > 0).sum() > 60, "the re-arm path was not exercised"


# ---- C. the option matrix ----------------------------------------------------------------------------------------------------
def both_references(m, table_name, n, k, T, tol, auto_reset, tape=None, **kw):
    tape = narrow_tape(T, n, len(_table(m, table_name)[0])) if tape is None else tape
    options = {key: kw[key] for key in ("substeps", "terminate_on_ground", "specialize") if key in kw}
    assert_tape_equals_per_step(m, table_name, n, k, tol, tape, auto_reset, episode0=kw.get("episode0", 0),
                                start_pose=kw.get("start_pose"), **options)
    return run_tape_against_oracle(m, table_name, n, k, T, tol, auto_reset, tape, **kw)


def test_terminate_on_ground_with_auto_reset(m):
    """done |= ground: every env finishes, most steps re-arm (oracle alone: clean 0.981, 19 815 re-arms, up to 12 episodes)."""
    stats = both_references(m, "ref", 3001, 7, 12, 20.0, True, terminate_on_ground=True)
    assert stats["finished"] == 3001 and stats["rearms"] > 15000 and stats["max_episodes"] == 12, stats
    stats["eng"].close()


def test_terminate_on_ground_without_auto_reset(m):
    """The done log is the ground flag (oracle alone: clean 0.975)."""
    stats = both_references(m, "ref", 3001, 7, 12, 8.0, False, terminate_on_ground=True)
    eng = stats["eng"]
    assert eng.get(m.lib.F_DONE).sum() > 0 and (eng.get(m.lib.F_DONE) != 0)[eng.reward() == -1].all()
    eng.close()


@pytest.mark.parametrize("substeps", [2, 3, 9, 24, 26])
def test_other_substep_counts(m, substeps):
    """Oracle alone: clean 0.997 / 0.997 / 0.996 / 0.988 / 0.986, 37 re-arms each."""
    stats = both_references(m, "ref", 3001, 7, 8, 20.0, True, substeps=substeps)
    assert stats["rearms"] > 18, stats
    stats["eng"].close()


def test_substeps_beyond_the_recurrence_are_refused(m):
    n, T = 3001, 3
    eng = make_engine(m, "ref", n, 7, 8.0)
    rotations = eng.dispatch()["policy"]["max_recurrence_rotations"]
    eng.close()
    last_ok = 2 * rotations + 2                        # engine.hip choose_dispatch: (S - 1) / 2 > rotations takes per-pose sincos
    assert last_ok == 26                               # (the S = 26 case above is the boundary's near side)
    eng = make_engine(m, "ref", n, 7, 8.0, substeps=last_ok + 1)
    eng.reset_random(SEED, 0)
    assert eng.dispatch()["tape"]["usable"] is False
    arg = m.lib.MtTape()
    tape = np.zeros((T * 4, n), dtype=np.float32)      # (never read: the call is refused on the host)
    arg.struct_size, arg.n_steps, arg.actions, arg.ld = C.sizeof(m.lib.MtTape), T, tape.ctypes.data, n
    rc = eng._lib.mt_rollout_tape(eng._h, C.byref(arg))
    msg = eng._lib.mt_last_error(eng._h).decode()
    assert rc == m.lib.MT_ERR_UNSUPPORTED and "substeps beyond the recurrence's reach" in msg, (rc, msg)
    with pytest.raises(m.ManytorError):
        eng.rollout_actions(np.zeros((T, n, 4), dtype=np.float32))
    eng.close()


def test_reference_table_as_a_runtime_table(m):
    """specialize=False: RtTable<4> on the reference's numbers, the inputs of the S = 2 case."""
    eng = make_engine(m, "ref", 3001, 7, 20.0, specialize=False, substeps=2)
    assert eng.dispatch()["table"] == "RtTable<4>", eng.dispatch()["table"]
    eng.close()
    stats = both_references(m, "ref", 3001, 7, 8, 20.0, True, substeps=2, specialize=False)
    assert stats["rearms"] > 18, stats
    stats["eng"].close()


@pytest.mark.parametrize("dof,rearms", [(3, 1258), (5, 1829), (8, 129)])
def test_generic_runtime_tables(m, dof, rearms):
    """RtTable<D>, radius 40, K = 3 (oracle alone: clean 0.970 / 0.992 / 0.993 and `rearms` re-arms)."""
    stats = both_references(m, f"dof{dof}", 3001, 3, 8, 20.0, True)
    assert stats["rearms"] > rearms // 2, stats
    stats["eng"].close()


def test_two_joints_bit_identity_only(m):
    """D = 2: with the default frames the observation row is the origin, z = 0 exactly: the oracle's ground margin is 0 for
    every env and none is clean (measured share 0.000), so the launch-per-step path is the only reference."""
    out = assert_tape_equals_per_step(m, "dof2", 3001, 3, 20.0, narrow_tape(8, 3001, 2), True)
    assert (out["finished"] > 0).sum() > 300             # (the oracle alone: 620 envs finish)


def test_one_target_full_reset_at_episode_7_ring_wraps(m):
    """K = 1, T = 24, ring of 8 slots, reset_random(SEED, 7): up to 15 episodes per env, slot (episode - 7) % 8 (oracle alone:
    clean 0.968, 16 663 re-arms)."""
    n = 3001
    stats = both_references(m, "ref", n, 1, 24, 30.0, True, episode0=7)
    eng = stats["eng"]
    assert stats["max_episodes"] > RING and stats["rearms"] > 8000 and stats["ring_written"] > 4 * n, stats
    assert eng.episode0 == 7
    np.testing.assert_array_equal(eng.episodes().astype(np.int64), 7 + eng.finished())
    np.testing.assert_array_equal(eng.finished()[stats["clean"]], stats["episodes"][stats["clean"]])
    eng.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_sizes_with_pitched_tape_and_logs(m, n):
    """Bit identity only (the oracle's clean share at n = 63 is 0.952: too close to MIN_CLEAN to be a fair condition).  The
    tape kernel returns early past n and then ballots `done` for MT_F_DONE_BITS; pad columns of the tape are NaN and never
    read, pad columns of the logs keep their fill."""
    import torch
    k, T, tol, D = 3, 12, 20.0, 4
    ld, log_ld = n + 37, n + 5
    tape = narrow_tape(T, n, D)
    a = make_engine(m, "ref", n, k, tol)
    b = make_engine(m, "ref", n, k, tol)
    for e in (a, b):
        e.reset_random(SEED, 0)
    state_a, outs_a, rew_a, done_a = run_per_step(m, a, tape, True)
    dev = torch.device("cuda", b.device)
    padded = torch.full((T * D, ld), float("nan"), dtype=torch.float32, device=dev)
    padded[:, :n] = torch.from_numpy(np.ascontiguousarray(tape.transpose(0, 2, 1)).reshape(T * D, n)).to(dev)
    rew = torch.full((T, log_ld), 0x55, dtype=torch.int8, device=dev)
    done = torch.full((T, log_ld), 0xAA, dtype=torch.uint8, device=dev)
    ret = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    arg = m.lib.MtTape()
    arg.struct_size, arg.n_steps, arg.actions, arg.ld = C.sizeof(m.lib.MtTape), T, padded.data_ptr(), ld
    arg.reward_log, arg.done_log, arg.log_ld, arg.return_out = rew.data_ptr(), done.data_ptr(), log_ld, ret.data_ptr()
    arg.seed, arg.flags = SEED, m.lib.TAPE_AUTO_RESET
    assert b._lib.mt_rollout_tape(b._h, C.byref(arg)) == m.lib.MT_OK, b._lib.mt_last_error(b._h)
    b.sync()
    rew, done = rew.cpu().numpy(), done.cpu().numpy()
    np.testing.assert_array_equal(rew[:, :n], rew_a)
    np.testing.assert_array_equal(done[:, :n], (done_a != 0).astype(np.uint8))
    assert (rew[:, n:] == 0x55).all() and (done[:, n:] == 0xAA).all()
    np.testing.assert_array_equal(ret.cpu().numpy(), rew_a.sum(axis=0).astype(np.float32))
    assert_same(snapshot(m, b, STATE), state_a, "state")
    want = dict(outs_a)
    want["F_DONE"] = np.where(outs_a["F_DONE"] != 0, 2, 0).astype(np.uint8)
    assert_same(snapshot(m, b, OUTPUTS), want, "outputs")                # (MT_F_DONE_BITS among them)
    bits = b.done_bits()
    unpacked = ((bits[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).ravel()
    np.testing.assert_array_equal(unpacked[:n], want["F_DONE"] != 0)
    assert not unpacked[n:].any()
    assert (b.finished() > 0).sum() > 0                                  # (the oracle alone: 1 / 10 / 19 / 22 / 65 envs finish)
    a.close()
    b.close()


@pytest.mark.parametrize("table_name,tol", [("ref", 20.0), ("dh7", 45.0)])
def test_start_pose_beyond_180_degrees_read_from_memory(m, table_name, tol):
    """eng.set(MT_F_GOALS) of poses out to +-32 460 degrees (turns_tape's recipe), then a narrow tape: the first step's route
    starts from a pose the kernel knows nothing about (pose_valid = false) and spans tens of thousands of degrees.  Oracle
    alone at T = 8: clean 0.988 (ref), 0.996 (dh7), so T stays 8."""
    n, T = 3001, 8
    D = len(_table(m, table_name)[0])
    pose = turns_tape(1, n, D)[0]
    assert np.abs(pose).max() > 30000
    stats = both_references(m, table_name, n, 7, T, tol, True, start_pose=pose)
    assert stats["rearms"] > (18 if table_name == "ref" else 280), stats       # (oracle alone: 37 / 570)
    stats["eng"].close()


@pytest.mark.parametrize("table_name,tol", [("ref", 20.0), ("dh7", 45.0)])
def test_one_tape_in_two_calls(m, table_name, tol):
    n, k, T, cut = 3001, 7, 12, 5
    whole = make_engine(m, table_name, n, k, tol)
    split = make_engine(m, table_name, n, k, tol)
    tape = narrow_tape(T, n, whole.dof)
    for e in (whole, split):
        e.reset_random(SEED, 0)
    kw = dict(auto_reset=True, seed=SEED, log=True, returns=True)
    one = whole.rollout_actions(tape, **kw)
    two = [split.rollout_actions(tape[:cut], **kw), split.rollout_actions(tape[cut:], **kw)]
    whole.sync()
    split.sync()
    assert_same(snapshot(m, split, EVERYTHING), snapshot(m, whole, EVERYTHING), "split vs whole")
    for key in ("reward", "done"):
        np.testing.assert_array_equal(np.concatenate([r[key].cpu().numpy() for r in two]), one[key].cpu().numpy(), err_msg=key)
    np.testing.assert_array_equal(two[0]["returns"].cpu().numpy() + two[1]["returns"].cpu().numpy(), one["returns"].cpu().numpy())
    assert (whole.finished() > 0).sum() > 60 and np.abs(one["reward"].cpu().numpy()).sum() > 0
    whole.close()
    split.close()


# ---- D. stream capture -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dry_run", [True, False], ids=["dry_run", "committing"])
def test_tape_call_is_capturable_in_a_hip_graph(m, dry_run):
    """include/manytor_hip.h: the call is legal under stream capture.  A linear capture on one side stream records
    `static_tape.copy_(staging); mt_rollout_tape` with preallocated log / return buffers; each of three replays with fresh tape
    contents equals the eager call on a twin: logs, returns and the state behind it."""
    import torch
    n, k, T, D, tol, replays = 20000, 7, 4, 4, 8.0, 3
    eager, graphed = make_engine(m, "ref", n, k, tol), make_engine(m, "ref", n, k, tol)
    for e in (eager, graphed):
        e.use_torch_stream()
        e.reset_random(SEED, 0)
    dev = torch.device("cuda", graphed.device)
    rows = np.ascontiguousarray(narrow_tape(replays * T, n, D).transpose(0, 2, 1)).reshape(replays, T * D, n)
    src = torch.from_numpy(rows).to(dev)
    staging = torch.zeros((T * D, n), dtype=torch.float32, device=dev)         # refreshed in front of every replay
    static_tape = torch.zeros((T * D, n), dtype=torch.float32, device=dev)
    rew = torch.zeros((T, n), dtype=torch.int8, device=dev)
    done = torch.zeros((T, n), dtype=torch.uint8, device=dev)
    ret = torch.zeros((n,), dtype=torch.float32, device=dev)
    arg = m.lib.MtTape()
    arg.struct_size, arg.n_steps, arg.actions, arg.ld = C.sizeof(m.lib.MtTape), T, static_tape.data_ptr(), n
    arg.reward_log, arg.done_log, arg.log_ld, arg.return_out = rew.data_ptr(), done.data_ptr(), n, ret.data_ptr()
    arg.seed, arg.flags = SEED, m.lib.TAPE_DRY_RUN if dry_run else 0
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        graphed.use_torch_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static_tape.copy_(staging)
            rc = graphed._lib.mt_rollout_tape(graphed._h, C.byref(arg))
    assert rc == m.lib.MT_OK, graphed._lib.mt_last_error(graphed._h)
    torch.cuda.synchronize(dev)
    graphed.reset_random(SEED, 0)         # the capture pass itself does not execute; start from the same state anyway
    torch.cuda.synchronize(dev)
    kw = dict(layout="soa", seed=SEED, log=True, returns=True, dry_run=dry_run)
    for r in range(replays):
        want = eager.rollout_actions(src[r].view(T, D, n), **kw)
        staging.copy_(src[r])
        graph.replay()
        torch.cuda.synchronize(dev)
        np.testing.assert_array_equal(rew.cpu().numpy(), want["reward"].cpu().numpy(), err_msg=f"replay {r}")
        np.testing.assert_array_equal(done.cpu().numpy(), want["done"].cpu().numpy(), err_msg=f"replay {r}")
        np.testing.assert_array_equal(ret.cpu().numpy(), want["returns"].cpu().numpy(), err_msg=f"replay {r}")
        assert np.abs(rew.cpu().numpy()).sum() > 0
        assert_same(snapshot(m, graphed, EVERYTHING), snapshot(m, eager, EVERYTHING), f"replay {r}")
    if dry_run:                           # nothing resident moved: the pose is still the reset's
        assert not graphed.goals().any() and graphed.bad_action_count() == 0
    else:
        np.testing.assert_array_equal(graphed.goals(), rows[-1].reshape(T, D, n)[-1].T)
    eager.close()
    graphed.close()
