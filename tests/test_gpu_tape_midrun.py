"""mt_rollout_tape in the MIDDLE of a run, held to the fp64 oracle.

A tape call is a writer the host has to know about: it leaves fractional joint angles (the whole-degree look-up of the next
sampled step's start pose would be wrong by up to 27 sin(0.5 deg) = 0.24), targets written as floats only (the 8-byte
target codes of the large batches no longer match), other returns than the overlapped gather's snapshot row holds, and with
auto_reset a new MT_F_LAST_RETURN; and it is an entry point like any other: forked chains are joined, a deferred
mt_reset_random is launched first.  tests/test_gpu_tape.py runs the call on a fresh handle only.  Here one script puts a tape
call in front of and behind every kind of call that keeps such knowledge, at every form mt_rollout takes (REGIMES of
tests/test_gpu_view_writes.py), on the handle's own stream and on torch's.

The oracle plays the script (Mirror of tests/test_gpu_view_writes.py: same program / replay / checkpoint machinery, same
tolerances, same guard-band rule).  A bit-identity twin (set_actions; step) would not do: it clears the same host flags by
another route, so a stale graph or table look-up in the calls that FOLLOW would show on both sides.

Between a library call and the call that consumes its state the host waits for nothing beyond what the Python front end
does itself (eng.rollout_actions on the handle's own stream: torch's stream before, the handle's after).  Where a segment
needs envs that finish -- at the default tolerance of 8 no env of a K = 7 batch picks all its targets in a few steps -- it
clears the alive bits of every fourth env through the MT_F_ALIVE view first (on the own stream between eng.sync() and
torch.cuda.synchronize(), as the header asks), which makes them finish in the next step."""
import numpy as np
import pytest

from test_gpu_view_writes import REGIMES, _assert_exercised, _make, replay

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def _tape(mir, T):
    """Fractional angles, uniform in +-180."""
    return mir.rng.uniform(-180.0, 180.0, size=(T, mir.n, mir.dof)).astype(np.float32)


def script_tape_mid_run(mir):
    t = 0
    mir.take_views("F_ALIVE")
    # 1. whole-degree poses, valid target codes, a cached graph / forked chains / a multi-step launch behind them
    mir.rollout(5, t)
    t += 5
    # 2. a tape, then the same rollout again: its start pose is fractional, its targets are floats, its StepArgs differ from
    #    the cached graph's, and on the own stream the chains of (1) were still forked when the tape call came
    tape = _tape(mir, 3)
    tape[1, 5, 0] = np.nan                                   # (one held pair: the counter runs mid-run as well)
    mir.rollout_actions(tape)
    before = mir.ora.total_reward.copy()
    mir.rollout(5, t)
    t += 5
    mir.gather_begin("first")                                # (allocates the snapshot rows: from here on mt_rollout's last launch
    mir.gather_end("first", stale=before)                    #  may store the returns there, which is what (5) is about)
    mir.check(label="2: tape(3), rollout(5)")
    # 3. in-kernel re-arms (new targets, floats only), then a sampled step, reset_done on what that step finished, a rollout
    mir.edit_kill(4)
    mir.rollout_actions(_tape(mir, 4), auto_reset=True)
    assert mir.episodes.sum() >= mir.n // 4                  # (re-armed inside the kernel)
    mir.edit_kill(6)
    mir.step_random(t)
    t += 1
    assert (mir.done == 1).sum() >= mir.n // 6
    mir.reset_done()
    mir.rollout(5, t)
    t += 5
    mir.check(label="3: tape(4, auto_reset), step_random, reset_done, rollout(5)")
    # 4. behind the fused rollout's own re-arms (done == 2 bytes, dead targets zeroed): a dry run right behind it, a dry run
    #    between two host snapshots, the committing call of the same rows
    mir.edit_kill(5)
    mir.rollout_fused(3, t, auto_reset=True)
    t += 3
    tape = _tape(mir, 3)
    dry0 = mir.rollout_actions(tape, dry_run=True, compare_resident=False)
    dry1 = mir.rollout_actions(tape, dry_run=True)
    real = mir.rollout_actions(tape)
    mir.expect_same_logs(dry0, real)
    mir.expect_same_logs(dry1, real)
    mir.check(label="4: rollout_fused(3, auto_reset), dry tape(3), tape(3)")
    # 5. the overlapped gather behind a tape: mt_rollout's last launch may have stored the returns to the snapshot row
    mir.rollout(5, t)
    t += 5
    before = mir.ora.total_reward.copy()
    mir.rollout_actions(_tape(mir, 2))
    mir.gather_begin("total")
    mir.gather_end("total", stale=before)
    mir.check(label="5: rollout(5), tape(2), gather_begin")
    # 6. an exchange that reads MT_F_LAST_RETURN in place, and a tape whose re-arms write that row
    mir.edit_kill(4)
    mir.gather_begin("last", field="F_LAST_RETURN", snapshot=False)
    mir.rollout_actions(_tape(mir, 3), auto_reset=True)
    mir.gather_end("last")
    # 7. a full reset at episode base 3 (deferred into the next mt_rollout where the handle does that), a tape in front of it
    mir.reset_random(3)
    mir.rollout_actions(_tape(mir, 3))
    mir.rollout(5, t)
    t += 5
    mir.check(label="7: reset_random(3), tape(3), rollout(5)")          # (episodes() among the fields)
    # 8. the two kernels that evaluate the resident pose, right behind a tape
    mir.rollout_actions(_tape(mir, 2))
    mir.observe()
    mir.check("observe", label="8: tape(2), observe")
    mir.rollout_actions(_tape(mir, 2))
    mir.check_done()
    mir.check("check_done", label="8: tape(2), check_done")


_SCRIPTED = {}      # regime -> the mirror that played the script: the oracle's run is shared by the two streams of a regime


CASES = [(r, False) for r in REGIMES] + [(r, True) for r in ("k5_lanes4", "graph", "large")]


@pytest.mark.parametrize("regime,on_torch_stream", CASES, ids=[f"{r}-{'torch' if s else 'own'}_stream" for r, s in CASES])
def test_tape_calls_mid_run_against_the_oracle(m, monkeypatch, regime, on_torch_stream):
    eng, mir = _make(m, monkeypatch, regime, on_torch_stream)
    d = eng.dispatch()
    assert d["tape"]["usable"] is True
    if regime == "large":
        # the launches of the first rollout read the targets as their 8-byte codes: the prefetch + trig-table step kernels of
        # a chain's range (engine.hip: plan_step), behind a full reset that was launched, not absorbed
        assert d["chains"]["prefetch"] is True and d["step"]["trig_table"] is True and d["rollout"]["absorbs_reset"] is False
        assert d["chains"]["span"] >= 131072, d["chains"]
    if regime not in _SCRIPTED:
        script_tape_mid_run(mir)
        _SCRIPTED[regime] = mir
    mir = _SCRIPTED[regime]                                  # (the program holds expectations only: replay leaves it as it is)
    replay(m, eng, mir, on_torch_stream)
    _assert_exercised(mir, REGIMES[regime]["k"])
    s = mir.stats
    assert s["dones"] > 0 and mir.bad_actions == 1, s        # (every regime: the script makes envs finish)
    assert mir.episode0 == 3
    eng.close()
