"""GPU tests of round 4: mt_rollout's k-steps-per-launch form, the per-chain mt_step / mt_set_actions / mt_sample_actions, the
dispatch as data (mt_describe_dispatch), the region timer, the streaming yardstick, the drop-in module name, and the
NaN / inf walk over every float-taking entry point of the C ABI.  Everything goes through ctypes -> C ABI -> HIP."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from parity_util import GUARD, POS_TOL, assert_obs_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_FIELDS = ("F_GOALS", "F_ALIVE", "F_TOTAL_REWARD", "F_POINTS", "F_EPISODES", "F_LAST_RETURN")
STEP_FIELDS = ("F_OBS", "F_REWARD", "F_DONE", "F_EE", "F_DONE_BITS")
RT5 = [[0, -1.2, 5, 0], [6, 0.37, 0, 0.2], [0, 1.57, 7, 0], [4, 0, 0, 0], [3, -1.57, 2, 0]]


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def snapshot(m, e, fields=STATE_FIELDS + STEP_FIELDS):
    return {f: e.get(getattr(m.lib, f)) for f in fields}


def assert_same(got, want, what=""):
    for f, v in want.items():
        np.testing.assert_array_equal(got[f], v, err_msg=f"{what}: {f}")


# ---- mt_rollout: k steps per launch -------------------------------------------------------------------
@pytest.mark.parametrize("chains", ["1", "2", "3"])
@pytest.mark.parametrize("rk", ["2", "4", "5", None])
@pytest.mark.parametrize("n,k,table_name", [(131072, 7, "ref"), (65536, 7, "ref"), (100003, 3, "ref"), (777, 9, "ref"),
                                            (70001, 7, "dh7"), (9001, 5, "rt5"), (262144, 7, "ref"), (3001, 32, "ref"),
                                            (200003, 1, "dh7"), (140000, 12, "ref")])
def test_rollout_k_steps_per_launch_equals_launch_per_step(m, monkeypatch, n, k, table_name, rk, chains):
    """On small shards (kPolicy.multi_step_max envs; any size with MT_ROLLOUT_K) mt_rollout runs k steps per launch through the rollout kernels (kPolicy.multi_step_*,
    MT_ROLLOUT_K; per chain on multi-chain handles).  State after the call and the outputs of its last step must equal
    the launch-per-step sequence bit for bit: segment lengths that are no multiple of k, ragged batches, both lane-split
    rollout kernels and the one-env-per-lane one, a reset_done queued right behind the segment, 2 and 3 chains."""
    table, radius = {"ref": (m.REF_DH_TABLE, 51.3), "dh7": (m.DH7_TABLE, 92.6), "rt5": (RT5, 25.0)}[table_name]
    if chains != "1" and n < 4096:
        pytest.skip("chains need a few blocks per range")
    monkeypatch.setenv("MT_ROLLOUT_K", "1")
    monkeypatch.setenv("MT_CHAINS", "1")
    monkeypatch.setenv("MT_GRAPH", "0")
    ref = m.StepEngine(n, k, dh_table=table, radius=radius, pickup_tol=20.0)
    assert ref.dispatch()["rollout"]["steps_per_launch"] == 1
    if rk is None:
        monkeypatch.delenv("MT_ROLLOUT_K")
    else:
        monkeypatch.setenv("MT_ROLLOUT_K", rk)
    monkeypatch.setenv("MT_CHAINS", chains)
    eng = m.StepEngine(n, k, dh_table=table, radius=radius, pickup_tol=20.0)
    d = eng.dispatch()
    multi = rk is not None or n <= d["policy"]["multi_step_max"]          # the default applies up to multi_step_max envs
    assert (d["rollout"]["form"] == "multi_step") == multi
    assert d["rollout"]["steps_per_launch"] == (int(rk or d["policy"]["multi_step_k"]) if multi else 1)
    assert d["chains"]["count"] == int(chains)
    assert (f"{d['rollout']['steps_per_launch']} steps per launch" in eng.step_kernel_name()) == multi
    step = 0
    for e in (ref, eng):
        e.reset_random(6, 0)
    for T in (9, 4, 1, 13, 2, 50):
        for e in (ref, eng):
            e.rollout(T, 6, step)
            if T == 13:
                e.reset_done(6)                  # queued on the handle's stream: must see every chain's last launch
        step += T
        assert_same(snapshot(m, eng), snapshot(m, ref), f"T={T}")
    ref.close()
    eng.close()


@pytest.mark.parametrize("kw", [dict(terminate_on_ground=True), dict(substeps=2), dict(substeps=24), dict(specialize=False),
                                dict(pickup_tol=60.0)])
def test_rollout_k_steps_per_launch_with_other_engine_options(m, monkeypatch, kw):
    """The multi-step form under the options that change what a step computes: ground contact ends the episode, the
    shortest and an even number of sub-steps, the runtime-table kernels of the reference arm, a pickup box that finishes
    episodes quickly -- each against the launch-per-step engine, with a reset_done in between."""
    n, k = 50000, 4
    monkeypatch.setenv("MT_ROLLOUT_K", "1")
    ref = m.StepEngine(n, k, **kw)
    monkeypatch.delenv("MT_ROLLOUT_K")
    eng = m.StepEngine(n, k, **kw)
    assert eng.dispatch()["rollout"]["form"] == "multi_step" and ref.dispatch()["rollout"]["steps_per_launch"] == 1
    for e in (ref, eng):
        e.reset_random(3, 0)
        e.rollout(11, 3, 0)
        e.reset_done(3)
        e.rollout(7, 3, 11)
    assert_same(snapshot(m, eng), snapshot(m, ref), str(kw))
    assert ref.done().any() or "substeps" in kw or "specialize" in kw
    ref.close()
    eng.close()


def test_rollout_default_dispatch_by_size(m, monkeypatch):
    """The regimes mt_create picks, asserted from mt_describe_dispatch's data against the library's own policy table
    (VERDICT r3 #7e: no name-string parsing)."""
    for v in ("MT_ROLLOUT_K", "MT_CHAINS", "MT_GRAPH", "MT_SPLIT", "MT_PREFETCH", "MT_FLAT_FROM", "MT_BLOCKS_PER_CU"):
        monkeypatch.delenv(v, raising=False)
    seen = {}
    for n in (1024, 32768, 49152, 65536, 131072, 163840, 262144, 262400, 393216, 786432, 1048576, 3145728, 3146752):
        e = m.StepEngine(n, 7)
        d = e.dispatch()
        P = d["policy"]
        seen[n] = d
        assert d["n_envs"] == n and d["table"] == "Ref4Table" and d["overrides"] == "" and d["trig"] == 0
        assert d["step"]["lanes_per_env"] == (4 if n <= P["step_split4_max"] else 2 if n <= P["step_split2_max"] else 1)
        assert d["step"]["prefetch"] == (d["step"]["lanes_per_env"] == 1) and d["step"]["trig_table"] is True
        assert d["step"]["flat"] == (n >= P["flat_from"])
        two = P["chains_min"] <= n <= P["chains_max"]
        assert d["chains"]["count"] == (2 if two else 1)
        span = (n // 2 + 255) // 256 * 256 if two else n
        assert d["chains"]["span"] == span and d["chains"]["lazy"] is True
        cap = next((c for lo, hi, c in P["block_caps"] if lo <= span < hi), 0) if two else 0
        assert d["chains"]["blocks_per_cu"] == cap
        assert d["chains"]["flat"] == (two and span >= P["flat_from"] or (not two and n >= P["flat_from"]))
        multi = n <= P["multi_step_max"]
        assert d["rollout"]["form"] == ("multi_step" if multi else "chained_steps" if two else "launch_per_step")
        assert d["rollout"]["steps_per_launch"] == (P["multi_step_k"] if multi else 1)
        assert d["rollout"]["absorbs_reset"] is multi and d["rollout"]["writes_snapshot"] is (multi or two)
        assert d["fused"]["usable"] is True
        assert d["fused"]["lanes_per_env"] == (4 if n <= P["fused_split4_max"] else 2 if n <= P["fused_split2_max"] else 1)
        assert d["reset"]["lanes_per_env"] == (4 if n <= P["reset_split_max"] else 1)
        assert d["ld"] == (n + 255) // 256 * 256 + (P["ld_pad_floats"] if n > P["ld_pad_above"] else 0)
        e.close()
    # the BASELINE shards: 1 M arms on one GPU = two chains of 524 288 with five blocks per CU and the FLAT form;
    # 131 072 (1 M over 8 GPUs) and 65 536 (configs[1]) = five steps per launch, two lanes per env
    assert seen[1048576]["chains"] == {"count": 2, "span": 524288, "lazy": True, "lanes_per_env": 1, "prefetch": True,
                                       "flat": True, "blocks_per_cu": 5}
    assert seen[131072]["rollout"] == {"form": "multi_step", "steps_per_launch": 5, "graph": False, "lanes_per_env": 2, "chains": 1, "absorbs_reset": True,
                                       "writes_snapshot": True}
    # 163 840 .. 262 144: a two-chain handle (mt_step, resets while forked) whose mt_rollout is multi-step on ONE chain
    assert seen[262144]["rollout"] == {"form": "multi_step", "steps_per_launch": 5, "graph": False, "lanes_per_env": 1, "chains": 1, "absorbs_reset": True,
                                       "writes_snapshot": True}
    assert seen[262144]["chains"]["count"] == 2 and seen[262400]["rollout"]["chains"] == 2
    assert seen[65536]["rollout"]["lanes_per_env"] == 2 and seen[32768]["rollout"]["lanes_per_env"] == 4
    # overrides are reported, and a 7-joint / runtime table / long route resolve differently
    monkeypatch.setenv("MT_ROLLOUT_K", "1")
    monkeypatch.setenv("MT_CHAINS", "3")
    e = m.StepEngine(100003, 7, dh_table=m.DH7_TABLE, radius=92.6)
    d = e.dispatch()
    assert d["overrides"] == "MT_CHAINS=3,MT_ROLLOUT_K=1" and d["table"] == "Dh7Table" and d["chains"]["count"] == 3
    assert d["rollout"] == {"form": "chained_steps", "steps_per_launch": 1, "graph": True, "lanes_per_env": 2, "chains": 3, "absorbs_reset": False,
                            "writes_snapshot": False}    # one cached graph per chain
    e.close()
    monkeypatch.delenv("MT_ROLLOUT_K")
    monkeypatch.delenv("MT_CHAINS")
    e = m.StepEngine(5000, 4, dh_table=RT5, radius=25.0, substeps=64)       # 31 rotations per half: no recurrence
    d = e.dispatch()
    assert d["table"] == "RtTable<5>" and d["trig"] == 1 and d["fused"]["usable"] is False
    assert d["rollout"]["form"] == "graph_replay" and d["rollout"]["steps_per_launch"] == 1 and d["step"]["lanes_per_env"] == 1
    e.close()


# ---- the episode boundary folded into mt_rollout's multi-step launches --------------------------------------------------
ALL_FIELDS = STATE_FIELDS + STEP_FIELDS + ("F_RETURN_RING",)


def _episode_script(m, e, name, seed, on_torch_stream=False):
    """Sequences around a full reset on a handle whose mt_rollout absorbs it; returns everything observable."""
    import torch
    out = {}
    if on_torch_stream:
        e.use_torch_stream()                             # stream order is the contract there: the reset is not deferred
    e.reset_random(seed, 0)
    if name == "loop":                                   # the benchmark's episode loop: rollout, overlapped gather, reset, rollout
        bufs = []
        for ep in range(1, 4):
            e.rollout(7 + ep, seed, 100 * ep)
            e.gather_wait()
            bufs.append(e.gather_begin())
            e.reset_random(seed, ep)
        e.rollout(6, seed, 900)
        e.gather_wait(host=True)
        e.sync()
        out["gathered"] = [b.cpu().numpy().copy() for b in bufs]
    elif name == "read_after_reset":                     # a getter right behind the reset: the reset's own state, complete
        e.rollout(9, seed, 0)
        e.reset_random(seed, 5)
        out["after_reset"] = snapshot(m, e, ALL_FIELDS)
        e.rollout(4, seed, 9)
    elif name == "reset_twice":                          # the second reset overwrites what the first one kept
        e.rollout(9, seed, 0)
        e.reset_random(seed, 1)
        e.reset_random(seed, 2)
        e.rollout(3, seed, 9)
    elif name == "staged_step":                          # the policy path behind a reset
        e.rollout(5, seed, 0)
        e.reset_random(seed, 1)
        e.sample_actions(seed, 77)
        e.step()
        e.rollout(3, seed, 78)
    elif name == "one_step_rollouts":                    # single-step rollouts: the first one absorbs the reset
        e.rollout(5, seed, 0)
        e.reset_random(seed, 1)
        e.rollout(1, seed, 5)
        e.rollout(1, seed, 6)
        e.rollout(4, seed, 7)
    elif name == "inplace_gather":                       # the exchange reads MT_F_LAST_RETURN, which the reset writes
        e.rollout(8, seed, 0)
        e.reset_random(seed, 1)
        buf = e.gather_begin(field=m.lib.F_LAST_RETURN, snapshot=False)
        e.rollout(5, seed, 8)
        e.reset_random(seed, 2)                          # must wait for the exchange (in the kernel that absorbs it, too)
        e.rollout(5, seed, 13)
        e.gather_wait(host=True)
        out["gathered"] = [buf.cpu().numpy().copy()]
    elif name == "device_view":                          # a raw view handed out behind a reset sees the reset
        e.rollout(6, seed, 0)
        e.reset_random(seed, 1)
        view = e.device_tensor(m.lib.F_TOTAL_REWARD)
        e.sync()
        out["view"] = view.clone().cpu().numpy()
        e.rollout(4, seed, 6)
    elif name == "fused_and_done":                       # other whole-batch calls behind the reset
        e.rollout(6, seed, 0)
        e.reset_random(seed, 1)
        e.rollout_fused(5, seed, 6, auto_reset=True)
        e.reset_random(seed, 2)
        e.reset_done(seed)
        e.rollout(5, seed, 11)
    elif name == "timers_and_single_step":               # timers do not launch a deferred reset; a one-step rollout absorbs it
        e.rollout(6, seed, 0)
        e.reset_random(seed, 1)
        e.timer_start()
        e.rollout(1, seed, 6)
        assert e.timer_stop() > 0.0
        e.reset_random(seed, 2)
        e.lap_begin()                                    # (a lap starts behind everything before it: launches the reset)
        e.rollout(3, seed, 7)
        e.lap_end()
        assert len(e.lap_times()) == 1
    else:
        raise AssertionError(name)
    torch.cuda.synchronize()
    out["final"] = snapshot(m, e, ALL_FIELDS)
    return out


@pytest.mark.parametrize("script", ["loop", "read_after_reset", "reset_twice", "staged_step", "one_step_rollouts", "inplace_gather",
                                    "device_view", "fused_and_done", "timers_and_single_step"])
@pytest.mark.parametrize("on_torch_stream", [False, True])
@pytest.mark.parametrize("n,k,table_name,chains", [(131072, 7, "ref", None), (3001, 9, "ref", None), (200003, 7, "ref", None),
                                                   (70001, 3, "dh7", None), (9001, 5, "rt5", None), (100003, 7, "ref", "2")])
def test_reset_and_snapshot_folded_into_rollout_launches_equal_the_eager_forms(m, monkeypatch, n, k, table_name, chains, script,
                                                                               on_torch_stream):
    """On a handle whose mt_rollout runs k steps per launch, mt_reset_random is deferred into the first launch of the next
    mt_rollout (RolloutArgs::reset_first) and the last launch of an mt_rollout also writes the overlapped gather's snapshot
    (RolloutArgs::snap).  Whatever is called in between -- getters, a second reset, staged steps, one-step rollouts, an
    in-place exchange of MT_F_LAST_RETURN, raw device views, fused rollouts, reset_done -- must see exactly what the eager
    reset kernel and the snapshot launch produce: every field, the gathered returns, the ring, bit for bit.  On a caller's
    stream the reset is not deferred (stream order is the contract there; test_step_is_capturable_in_a_hip_graph replays a
    captured step right behind a reset) and mt_rollout leaves the snapshot to mt_gather_returns_begin, which copies the row in
    stream order (a torch write between the two calls is gathered: test_gpu_view_writes.py)."""
    table, radius = {"ref": (m.REF_DH_TABLE, 51.3), "dh7": (m.DH7_TABLE, 92.6), "rt5": (RT5, 25.0)}[table_name]
    if chains:
        monkeypatch.setenv("MT_CHAINS", chains)
    monkeypatch.setenv("MT_DEFER_RESET", "0")
    monkeypatch.setenv("MT_ROLLOUT_SNAP", "0")
    ref = m.StepEngine(n, k, dh_table=table, radius=radius, pickup_tol=20.0, return_ring=3)
    assert ref.dispatch()["rollout"]["absorbs_reset"] is False and ref.dispatch()["rollout"]["writes_snapshot"] is False
    want = _episode_script(m, ref, script, 17, on_torch_stream)
    ref.close()
    monkeypatch.delenv("MT_DEFER_RESET")
    monkeypatch.delenv("MT_ROLLOUT_SNAP")
    eng = m.StepEngine(n, k, dh_table=table, radius=radius, pickup_tol=20.0, return_ring=3)
    d = eng.dispatch()["rollout"]
    assert d["form"] == "multi_step" and d["absorbs_reset"] is True and d["writes_snapshot"] is True
    got = _episode_script(m, eng, script, 17, on_torch_stream)
    eng.close()
    assert_same(got["final"], want["final"], script)
    if "after_reset" in want:
        assert_same(got["after_reset"], want["after_reset"], script + ": right behind the reset")
        a = want["after_reset"]
        assert not a["F_GOALS"].any() and not a["F_TOTAL_REWARD"].any() and a["F_ALIVE"].all() and (a["F_EPISODES"] == 5).all()
    for key in ("gathered",):
        for x, y in zip(got.get(key, []), want.get(key, [])):
            np.testing.assert_array_equal(x, y, err_msg=f"{script}: {key}")
            assert np.abs(y).max() > 0
    if "view" in want:
        np.testing.assert_array_equal(got["view"], want["view"])
        assert not want["view"][:n].any()


@pytest.mark.parametrize("script", ["loop", "read_after_reset", "reset_twice", "staged_step", "one_step_rollouts", "inplace_gather",
                                    "device_view", "fused_and_done", "timers_and_single_step"])
@pytest.mark.parametrize("n,k,table_name,env", [(300007, 7, "ref", {}), (530000, 5, "dh7", {}),
                                                (70001, 3, "ref", {"MT_CHAINS": "3", "MT_ROLLOUT_K": "1", "MT_GRAPH": "0"})])
def test_reset_folded_into_the_first_launch_of_each_chain_equals_the_eager_form(m, monkeypatch, n, k, table_name, env, script):
    """The chained launch-per-step form of the large batches: the last step launch of every chain writes the overlapped
    gather's snapshot (default), and with MT_DEFER_RESET_CHAINS=1 a deferred mt_reset_random becomes the prologue of ONE step
    of the rollout kernel at the head of each chain's launches -- the same scripts, the same bits as the eager per-chain
    reset kernels and snapshot copies."""
    table, radius = {"ref": (m.REF_DH_TABLE, 51.3), "dh7": (m.DH7_TABLE, 92.6)}[table_name]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    monkeypatch.setenv("MT_DEFER_RESET", "0")
    monkeypatch.setenv("MT_ROLLOUT_SNAP", "0")
    ref = m.StepEngine(n, k, dh_table=table, radius=radius, pickup_tol=20.0, return_ring=3)
    d = ref.dispatch()["rollout"]
    assert d["absorbs_reset"] is False and d["writes_snapshot"] is False and d["form"] == "chained_steps"
    want = _episode_script(m, ref, script, 23)
    ref.close()
    monkeypatch.delenv("MT_DEFER_RESET")
    monkeypatch.delenv("MT_ROLLOUT_SNAP")
    monkeypatch.setenv("MT_DEFER_RESET_CHAINS", "1")
    eng = m.StepEngine(n, k, dh_table=table, radius=radius, pickup_tol=20.0, return_ring=3)
    d = eng.dispatch()["rollout"]
    assert d["form"] == "chained_steps" and d["graph"] is False and d["absorbs_reset"] is True and d["writes_snapshot"] is True
    got = _episode_script(m, eng, script, 23)
    eng.close()
    assert_same(got["final"], want["final"], script)
    if "after_reset" in want:
        assert_same(got["after_reset"], want["after_reset"], script + ": right behind the reset")
    for x, y in zip(got.get("gathered", []), want.get("gathered", [])):
        np.testing.assert_array_equal(x, y, err_msg=f"{script}: gathered")
        assert np.abs(y).max() > 0
    if "view" in want:
        np.testing.assert_array_equal(got["view"], want["view"])


@pytest.mark.parametrize("n,throttle", [(131072, "1"), (131072, "0"), (40001, "1"), (300007, "1")])
def test_unfenced_episode_loop_gathers_every_episode_exactly(m, monkeypatch, n, throttle):
    """A learner's loop without host fences: 40 episodes queued back to back, every episode's returns gathered on the side
    stream into a buffer of its own, nothing waited for until the end.  The snapshot rows alternate (double buffer) and
    mt_gather_returns_begin keeps the host one exchange ahead at most (MT_GATHER_THROTTLE=0: never waits, the snapshot
    falls back to a launch of its own) -- every gathered vector must be that episode's returns, i.e. what the same seeds
    give on a handle that gathers in line (mt_gather_returns, no side stream)."""
    import torch
    monkeypatch.setenv("MT_GATHER_THROTTLE", throttle)
    eng = m.StepEngine(n, 7, pickup_tol=20.0)
    assert ("MT_GATHER_THROTTLE=" + throttle) in eng.dispatch()["overrides"]
    monkeypatch.delenv("MT_GATHER_THROTTLE")
    ref = m.StepEngine(n, 7, pickup_tol=20.0)
    E, L = 40, 11
    got, want = [], []
    for e, out, overlapped in ((eng, got, True), (ref, want, False)):
        e.reset_random(5, 0)
        for ep in range(E):
            e.rollout(L, 5, ep * L)
            out.append(e.gather_begin() if overlapped else e.gather_returns())
            e.reset_random(5, ep + 1)
        e.gather_wait(host=True) if overlapped else None
        e.sync()
    torch.cuda.synchronize()
    distinct = set()
    for ep, (x, y) in enumerate(zip(got, want)):
        a, b = x.cpu().numpy(), y.cpu().numpy()
        np.testing.assert_array_equal(a, b, err_msg=f"episode {ep}")
        distinct.add(a.tobytes())
    assert len(distinct) > E // 2                        # the episodes differ: a stale snapshot row would repeat one
    eng.close()
    ref.close()


# ---- mt_step per chain --------------------------------------------------------------------------------
def _policy_steps(m, e, torch, mode, seed, steps, on_torch_stream):
    """`steps` policy-in-the-loop steps; the actions reach the engine by `mode`."""
    n, d = e.n_envs, e.dof
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    for t in range(steps):
        if mode == "sample":
            e.sample_actions(seed, t)
            e.step()
            continue
        a = (torch.rand((n, d), generator=g, device="cuda") * 360.0 - 180.0)
        if t == 3:
            a[5::1000, 1] = float("nan")                 # a diverging policy: those envs hold their pose
        if mode == "env_major_f32":
            e.step(a)
        elif mode == "env_major_f64":
            e.step(a.double())
        elif mode == "env_major_i64":
            e.step(a.round().long())
        elif mode == "soa_f32":
            soa = torch.zeros((d, e.ld), device="cuda")
            soa[:, :n] = a.t()
            e.step(soa)
        elif mode == "view":                             # zero-copy: the policy writes the (D, N) view of the action rows
            view = e.device_tensor(m.lib.F_ACTIONS)
            view.copy_(a.t())
            if not on_torch_stream:
                torch.cuda.synchronize()                 # own stream: ordered against nothing, the caller syncs
            e.step()
        else:
            raise AssertionError(mode)


@pytest.mark.parametrize("on_torch_stream", [False, True])
@pytest.mark.parametrize("mode", ["sample", "env_major_f32", "env_major_f64", "env_major_i64", "soa_f32", "view"])
@pytest.mark.parametrize("n,k,chains", [(300003, 7, None), (1048576, 7, None), (70001, 3, "2"), (9001, 5, "3"), (524288, 2, "4")])
def test_chained_mt_step_equals_single_launch(m, monkeypatch, n, k, chains, mode, on_torch_stream):
    """mt_step on a multi-chain handle is one launch per env range on its own stream, and mt_sample_actions /
    mt_set_actions(device) stage each range's rows on the same streams -- on the handle's own stream the chains stay forked
    from call to call, on torch's stream every call forks behind the policy's kernels and joins back.  Every field must
    equal the single-launch engine bit for bit: ragged and large batches, every device action form, unusable actions
    counted once, and whole-batch calls (reset_done, getters) right behind the per-chain ones."""
    import torch
    monkeypatch.setenv("MT_CHAINS", "1")
    ref = m.StepEngine(n, k, pickup_tol=20.0)
    if chains is None:
        monkeypatch.delenv("MT_CHAINS")
    else:
        monkeypatch.setenv("MT_CHAINS", chains)
    eng = m.StepEngine(n, k, pickup_tol=20.0)
    assert eng.dispatch()["chains"]["count"] == int(chains or 2) and ref.dispatch()["chains"]["count"] == 1
    for e in (ref, eng):
        if on_torch_stream:
            e.use_torch_stream()
        e.reset_random(11, 0)
        _policy_steps(m, e, torch, mode, 11, 6, on_torch_stream)
        e.reset_done(11)                                 # whole-batch call right behind per-chain work
        _policy_steps(m, e, torch, mode, 12, 3, on_torch_stream)
    assert_same(snapshot(m, eng, STATE_FIELDS + STEP_FIELDS + ("F_ACTIONS",)), snapshot(m, ref, STATE_FIELDS + STEP_FIELDS + ("F_ACTIONS",)), mode)
    assert eng.bad_action_count() == ref.bad_action_count()
    if mode == "sample":
        assert eng.bad_action_count() == 0
    elif mode != "env_major_i64":                        # (what a NaN becomes as an int64 is the caster's business)
        assert eng.bad_action_count() > 0
    if on_torch_stream:                                  # a torch read right behind a step sees every range (the call joined)
        eng.sample_actions(5, 0)
        ref.sample_actions(5, 0)
        eng.step()
        ref.step()
        got = eng.device_tensor(m.lib.F_TOTAL_REWARD).clone()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy(), ref.total_reward())
    ref.close()
    eng.close()


def test_chained_mt_step_every_env_against_the_c_oracle(m):
    """The default dispatch of the policy-in-the-loop path at BASELINE's size (1 048 576 arms: two chains of 524 288, FLAT
    staged-action kernel), fractional-degree actions through the zero-copy view: every env against the C oracle."""
    import torch
    from oracle import c_oracle
    from oracle import philox_ref as px
    n, k = 1048576, 7
    eng = m.StepEngine(n, k)
    d = eng.dispatch()
    assert d["chains"]["count"] == 2 and d["chains"]["flat"] is True
    eng.reset_random(0x5EED, 0)
    ids = np.arange(n, dtype=np.uint64)
    pts = eng.points()
    np.testing.assert_array_equal(pts[:4096], px.sample_targets(0x5EED, ids[:4096], 0, k, 51.3))
    ora = c_oracle.COracle(n, k, threads=16)
    ora.reset(pts.astype(np.float64))
    view = eng.device_tensor(m.lib.F_ACTIONS)
    g = torch.Generator(device="cuda")
    g.manual_seed(4)
    guarded = 0
    for t in range(4):
        a = (torch.rand((4, n), generator=g, device="cuda") * 360.0 - 180.0)
        view.copy_(a)
        torch.cuda.synchronize()
        eng.step()
        act = a.t().contiguous().cpu().numpy()
        pre_alive = ora.alives.copy()
        obs_ref, rew_ref, done_ref = ora.step(act.astype(np.float64))
        np.testing.assert_array_equal(eng.goals(), act)
        assert np.abs(eng.joints_coordinates() - ora.joints_coordinates).max() <= POS_TOL
        pm = np.where(pre_alive, ora.pickup_margin, np.inf).min(axis=1)
        risky = (ora.ground_margin < GUARD) | (pm < GUARD)
        ok = ~risky
        guarded += int(risky.sum())
        np.testing.assert_array_equal(eng.reward()[ok], rew_ref[ok])
        np.testing.assert_array_equal(eng.done()[ok], done_ref[ok])
        alive_gpu = eng.alives()
        np.testing.assert_array_equal(alive_gpu[ok], ora.alives[ok])
        assert_obs_close(eng.obs(), obs_ref, ora.joints_coordinates[:, -2], ora.points, pre_alive)
        idx = np.flatnonzero(risky)                      # re-synchronise the few envs inside the guard band
        ora.alive_u8[idx] = alive_gpu[idx]
        ora.total_reward[idx] = eng.total_reward()[idx]
        ora.points[idx] = eng.points()[idx].astype(np.float64)
        np.testing.assert_array_equal(eng.total_reward(), ora.total_reward.astype(np.float32))
    assert guarded < 4 * n * 3e-3 + 8, guarded        # measured 2.2e-3 of the env-steps with fractional-degree actions
    eng.close()


# ---- timers / probe ---------------------------------------------------------------------------------------------------
def test_async_timer_covers_chains_and_a_pending_exchange(m, monkeypatch):
    """mt_timer_stop_async + mt_timer_read: the span from the start mark to the LAST end event over the handle's stream,
    its forked chains and an exchange pending on the side stream -- without joining or waiting in between.  Must read
    like the joined timer over the same work (not like half of it), and the chains must still be forked afterwards."""
    n, k, T = 1048576, 7, 20
    monkeypatch.setenv("MT_CHAINS", "2")
    e = m.StepEngine(n, k)
    e.reset_random(1, 0)
    for _ in range(5):
        e.rollout(50, 1, 0)
    e.sync()
    spans, joined = [], []
    for r in range(8):
        e.reset_random(1, r)
        e.sync()
        e.timer_start()
        e.rollout(T, 1, 0)                                   # leaves the chains forked
        buf = e.gather_begin()                               # snapshot per chain + exchange on the side stream
        e.timer_stop_async()
        spans.append(e.timer_read())
        e.gather_wait(host=True)
        assert buf.numel() == n
        e.sync()
        e.timer_start()
        e.rollout(T, 1, T)
        joined.append(e.timer_stop())
    span, ref = np.median(spans), np.median(joined)
    assert 0.8 * ref <= span <= 1.35 * ref, (span, ref)       # + the snapshot copy and the 4 MB device copy of the "exchange"
    assert span * 1e3 / T > 25.0
    with pytest.raises(m.ManytorError):
        e.timer_read()                                       # nothing to read twice
    e.close()


def test_stream_probe_moves_the_steps_bytes(m):
    """mt_stream_probe: 233 B per env for the reference arm with 7 targets, 257 B for the 7-joint arm, a plausible rate,
    and a loud refusal for shapes it was not built for."""
    us, nbytes = m.stream_probe(1048576, 4, 7, reps=20)
    assert nbytes == 233 * 1048576 and 20.0 < us < 200.0
    gbs = nbytes / (us * 1e-6) / 1e9
    assert 1200.0 < gbs < 9000.0, gbs
    us7, nbytes7 = m.stream_probe(262144, 7, 7, reps=20)
    assert nbytes7 == 257 * 262144 and us7 > 0
    with pytest.raises(m.ManytorError):
        m.stream_probe(4096, 5, 7)


# ---- the drop-in module name (VERDICT r3 #7c) -------------------------------------------------------------------------
def test_import_manytor_as_tor_runs_the_test_multi_loop(golden):
    """`import manytor as tor` -- what /root/reference/test_multi.py:1 resolves to when this repository is on the path --
    and the loop of test_multi.py:11-34 on fixture F4's seed: same actions, per-epoch returns read through
    `multienv.environment[i].total_reward` (test_multi.py:32), `done == True` never breaking (:22), the render toggle
    of every 10th epoch a no-op without a viewer (:25-28)."""
    sys.path.insert(0, ROOT)
    import manytor as tor
    assert tor.__file__ == os.path.join(ROOT, "manytor.py") and tor.Multienv.__module__ == "manytor_amd.api"
    g = golden("f4_multienv_trace")
    env_shape = tuple(int(v) for v in g["env_shape"])
    obj_number, max_steps = int(g["obj_number"]), int(g["max_steps"])
    np.random.seed(int(g["seed"]))
    multienv = tor.Multienv(env_shape, obj_number)
    obs = multienv.reset(returnable=True)
    assert len(obs) == multienv.env_number == 6
    t = 0
    for i in range(1, len(g["total_reward"]) + 1):
        broke = False
        for p in range(max_steps):
            action = multienv.action_sample()
            np.testing.assert_array_equal(np.array(action), g["action"][t])
            obs2, reward, done = multienv.step(action)
            t += 1
            if done == True:  # noqa: E712  (test_multi.py:22, verbatim: a list is never == True)
                broke = True
                break
        assert not broke and p == max_steps - 1
        if i % 10 == 0:
            multienv.render(stop_render=multienv.rendering)
        totals = [multienv.environment[k].total_reward for k in range(multienv.env_number)]
        assert all(isinstance(v, float) for v in totals)
        np.testing.assert_array_equal(np.array(totals), g["total_reward"][i - 1])      # no guarded case on this fixture
        jc = np.array([e.joints_coordinates for e in multienv.environment])
        assert np.abs(jc - g["jc"][t - 1]).max() <= POS_TOL
        multienv.reset()
    assert t == 2 * max_steps
    multienv.render(stop_render=True)
    # the module functions under the reference's names
    np.testing.assert_allclose(tor.fk(4, [30, 45, -60, 90])[0:3, 3], [34.839021, -6.885682, 11.936753], atol=POS_TOL)
    assert tor.HOST == "localhost" and tor.PORT == 5001


# ---- NaN / inf at every float-taking entry point (VERDICT r3 #7f) -----------------------------------------------------
# What each entry point of include/manytor_hip.h that takes floating-point DATA does with a NaN / an infinity.  The test
# below walks the header: a new float-taking function that is not listed here fails it.
FLOAT_ENTRY_POINTS = {
    "mt_create": "rejects (pickup_tol, radius, dh_table)",
    "mt_reset": "rejects host arrays; drops + counts unusable targets handed over in device memory",
    "mt_env_reset": "rejects",
    "mt_set_actions": "accepted: the env holds its pose for the step, counted (mt_bad_action_count)",
    "mt_step_host": "accepted: the env holds its pose for the step, counted",
    "mt_env_step": "accepted: the env holds its pose for the step, counted",
    "mt_set": "rejects (GOALS, POINTS, TOTAL_REWARD, LAST_RETURN, RETURN_RING)",
    "mt_fk_batch": "rejects",
    "mt_route_trace": "rejects",
    "mt_r_theta_batch": "rejects",
    # float* OUTPUTS only (nothing to screen): listed so that the walk is complete
    "mt_gather_returns": "output", "mt_gather_returns_begin": "output", "mt_gather_returns_begin_inplace": "output",
    "mt_gather_returns_wait": "output", "mt_timer_stop": "output", "mt_timer_read": "output", "mt_timer_laps_total": "output",
    "mt_timer_lap_times": "output", "mt_stream_probe": "output", "mt_get": "output (void*)", "mt_reduce_returns": "output",
}


def float_taking_functions():
    text = open(os.path.join(ROOT, "include", "manytor_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for mm in re.finditer(r"MT_API\s+[\w\s\*]+?\b(mt_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        name, args = mm.group(1), mm.group(2)
        if re.search(r"\bfloat\b|\bdouble\b|const\s+void\s*\*\s*(actions|src)|mt_config|mt_return_stats|void\s*\*\s*dst", args):
            out[name] = args
    return out


@pytest.mark.parametrize("poison", [float("nan"), float("inf"), -float("inf")])
def test_nan_and_inf_at_every_float_taking_entry_point(m, poison):
    """-ffinite-math-only safety net: no NaN / infinity reaches the kernels' arithmetic through any entry point.  Host
    arrays are refused before anything is written; what can only be seen on the device (staged actions, device targets)
    is neutralised and counted; and the engine's state stays finite and steppable after every attempt."""
    lib, L = m.lib.load(), m.lib
    funcs = float_taking_functions()
    assert set(funcs) == set(FLOAT_ENTRY_POINTS), sorted(set(funcs) ^ set(FLOAT_ENTRY_POINTS))
    import torch
    n, k, d = 1000, 3, 4
    eng = m.StepEngine(n, k, return_ring=2)
    eng.reset_random(1, 0)
    eng.rollout(3, 1, 0)
    before = snapshot(m, eng, STATE_FIELDS)

    # mt_create
    for field in ("pickup_tol", "radius", "dh_table"):
        cfg = L.MtConfig()
        cfg.struct_size = C.sizeof(L.MtConfig)
        cfg.n_envs, cfg.dof, cfg.n_targets, cfg.substeps = 64, 4, 2, 25
        cfg.pickup_tol, cfg.radius, cfg.obs_frame, cfg.ee_frame = 8.0, 51.3, -2, -1
        for j, row in enumerate(m.REF_DH_TABLE):
            for q, v in enumerate(row):
                cfg.dh_table[4 * j + q] = v
        if field == "dh_table":
            cfg.dh_table[6] = poison
        else:
            setattr(cfg, field, poison)
        h = L._HANDLE()
        assert lib.mt_create(C.byref(h), C.byref(cfg)) == L.MT_ERR_INVALID_ARG and not h.value, field

    # mt_reset / mt_env_reset / mt_set: host arrays are refused, nothing is written
    pts = np.random.default_rng(0).uniform(1, 20, (n, k, 3)).astype(np.float32)
    bad = pts.copy()
    bad[17, 1, 2] = poison
    with pytest.raises(ValueError):
        eng.reset(bad)
    soa = np.zeros((3 * k, eng.ld), dtype=np.float32)
    soa[:, :n] = bad.reshape(n, 3 * k).T
    assert lib.mt_reset(eng._h, soa.ctypes.data_as(C.c_void_p), L.SOA, 0) == L.MT_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        eng.env_reset(5, points=bad[17])
    for f, arr in ((L.F_GOALS, eng.goals()), (L.F_POINTS, eng.points()), (L.F_TOTAL_REWARD, eng.total_reward()),
                   (L.F_LAST_RETURN, eng.last_return()), (L.F_RETURN_RING, eng.return_ring())):
        a = np.array(arr, dtype=np.float32)
        a.flat[a.size // 2] = poison
        with pytest.raises(ValueError):
            eng.set(f, a)
    assert_same(snapshot(m, eng, STATE_FIELDS), before, "after the refused calls")

    # stateless helpers
    with pytest.raises(ValueError):
        m.fk_batch(4, np.array([[0, poison, 0, 0]], dtype=np.float32))
    with pytest.raises(ValueError):
        m.route_trace(np.zeros((1, 4), np.float32), np.array([[0, 0, poison, 0]], np.float32))
    with pytest.raises(ValueError):
        m.r_theta_batch(np.array([[0, 0, poison]], np.float32), np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError):
        m.fk_batch(4, np.zeros((1, 4), np.float32), dh_table=[[0, poison, 4.3, 0]] + [list(r) for r in m.REF_DH_TABLE[1:]])

    # staged actions: accepted, the env holds its pose, counted -- every entry that stages one
    count0 = eng.bad_action_count()
    g0 = eng.goals()
    act = np.random.default_rng(1).integers(-180, 180, (n, d)).astype(np.float32)
    act[3, 2] = poison
    eng.step(act)                                            # mt_set_actions (host) + mt_step
    np.testing.assert_array_equal(eng.goals()[3], g0[3])
    assert eng.bad_action_count() == count0 + 1
    g1 = eng.goals()
    eng.step(torch.from_numpy(act).cuda())                   # mt_set_actions (device)
    np.testing.assert_array_equal(eng.goals()[3], g1[3])
    obs, rew, done = eng.step_host(act)                      # mt_step_host
    assert np.isfinite(obs).all() and eng.bad_action_count() == count0 + 3
    g2 = eng.goals()
    o1, r1, d1 = eng.env_step(9, [0.0, poison, 0.0, 0.0])    # mt_env_step
    np.testing.assert_array_equal(eng.goals()[9], g2[9])
    assert np.isfinite(o1).all() and eng.bad_action_count() == count0 + 4

    # targets in device memory: the reset kernel drops the unusable ones and counts them
    dev_pts = torch.from_numpy(bad).cuda()
    eng._call(lib.mt_reset, C.c_void_p(dev_pts.data_ptr()), L.ENV_MAJOR, 1)
    eng.sync()
    p = eng.points()
    assert np.isfinite(p).all() and not p[17, 1].any() and not eng.alives()[17, 1] and eng.alives().sum() == n * k - 1
    assert eng.bad_action_count() == count0 + 5
    np.testing.assert_array_equal(np.delete(p.reshape(-1, 3), 17 * k + 1, axis=0), np.delete(bad.reshape(-1, 3), 17 * k + 1, axis=0))

    # and the engine is still finite and steppable
    eng.rollout(5, 2, 0)
    eng.rollout_fused(5, 2, 5)
    for f, v in snapshot(m, eng, ("F_GOALS", "F_POINTS", "F_TOTAL_REWARD", "F_OBS", "F_EE", "F_LAST_RETURN", "F_RETURN_RING")).items():
        assert np.isfinite(v).all(), f
    eng.close()
