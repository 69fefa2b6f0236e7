"""CPU checks of tests/call_sequences.py, ahead of anything that needs a GPU: the generated sequences hold every op of the
alphabet in both positions, no stretch between two full resets is longer than MAX_STEPS env-steps, and the oracle leg's
sequences, played by the fp64 oracle alone, keep the share of envs that entered the guard band under the cap the GPU test
asserts at every comparison point (random fractional actions stand in for the policies' and the planners'; for the staged
IK op the fp64 solver itself does, which also shows that both of its appearances have targets to reach for).  Last, every
public method of StepEngine is called by an op of the alphabet or is exempt by name, with a reason."""
import numpy as np
import pytest

import call_sequences as cs
from parity_util import GUARD

SHUFFLES = (0, 1, 2)
SIZES = (5003, 70144)      # without and with the two population ops (n / 2 a multiple of 256)
CAP = 0.10


@pytest.mark.parametrize("oracle", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shuffle", SHUFFLES)
def test_every_op_in_both_positions(shuffle, n, oracle):
    head, groups = cs.generate(shuffle, n, oracle)
    assert list(head) == [("reset_random", 0), ("rollout", 3, 0)]
    ops = cs.alphabet(n, oracle)
    assert ("rollout_population" in ops) == cs.population_ok(n)
    assert ("es" in ops) == (cs.population_ok(n) and not oracle)
    assert set(cs.MOVING) <= set(ops) and set(cs.NOTHING) <= set(ops)
    assert {"jacobian", "ik", "ik(stage)+step"} <= set(ops)
    assert {"jacobian", "ik"} <= set(cs.NOTHING) & set(cs.KEEPERS) and cs.MOVING["ik(stage)+step"] == 1
    for with_reset in (False, True):
        assert sorted(g.op for g in groups if g.with_reset == with_reset) == sorted(ops)
    t = 3
    saved = False
    for g in groups:
        # directly in front of the op: a full reset, or none
        assert (bool(g.pre) and g.pre[-1][0] == "reset_random") == g.with_reset, g
        if g.with_reset:
            assert g.pre[-2][:2] == ("rollout", 2), g            # ... which finds the chains forked
        assert g.trail and all(it[0] in ("rollout", "step_random") for it in g.trail)
        # the sampled calls continue the step index, whatever ran between
        for it in g.pre + ((("op", g.t),) if g.op in cs.SAMPLED_OPS else ()) + g.trail:
            if it[0] == "rollout":
                assert it[2] == t and 1 <= it[1] <= 3
                t += it[1]
            elif it[0] == "step_random":
                assert it[1] == t
                t += 1
            elif it[0] == "op":
                assert it[1] == t
                t += cs.SAMPLED_OPS[g.op]
            saved |= it[0] == "save_state"
        if g.op == "set_state":
            assert saved
        if g.op in cs.LOG_USERS:
            assert any(p.op in cs.LOG_MAKERS for p in groups[:groups.index(g)])
    tails = [g.trail[-1] for g in groups]
    assert {it[1] for it in tails if it[0] == "rollout"} == {1, 2, 3} and any(it[0] == "step_random" for it in tails)


@pytest.mark.parametrize("oracle", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shuffle", SHUFFLES)
def test_no_stretch_between_full_resets_exceeds_the_limit(shuffle, n, oracle):
    lengths = cs.stretches(*cs.generate(shuffle, n, oracle))
    assert max(lengths) <= cs.MAX_STEPS, lengths
    assert max(lengths) >= 30                    # ... and some stretches are long enough for most envs to finish


def test_samples_hold_the_edges():
    for n, span in ((5003, 5003), (300007, 150016), (70001, 70001)):
        s = cs.sample_of(n, span)
        assert len(s) <= 4100 and s[0] == 0 and s[-1] == n - 1
        assert set(cs.single_envs(n, span)) <= set(s.tolist())
        if span < n:
            assert span - 1 in s and span in s


@pytest.mark.parametrize("n", SIZES)
def test_the_oracle_alone_stays_under_the_guard_band_cap(n):
    """The oracle leg's sequence (shuffle 0, the one the GPU test plays) on 1 000 envs: at every comparison point fewer than
    10 % of them have come within GUARD of a threshold since the last full reset.  (1 000: the fp64 oracle costs 40 us per
    env-step; a share near 5 % is then known to +-0.7 points, far from the cap.)"""
    m_ = 1000
    span = n // 2 // 256 * 256
    sample = np.unique(np.concatenate([cs.sample_of(n, span)[:m_ - 4], cs.single_envs(n, span)]))
    data = cs.Data(n, span)
    fo = cs.OracleFollower(sample, data, GUARD)
    rng = np.random.default_rng(3)
    reaching = []                    # per appearance of ik(stage)+step: the share of envs with a target that move towards it

    def stand_in(op):
        if op == "ik(stage)+step":   # a reach controller drives arms ONTO targets, which random angles do not: the solver itself
            angles, _, steps, index = fo.reach(cs.REACH_ITERS, cs.REACH_TOL)
            reaching.append(((index >= 0) & (steps > 0)).mean())
            return angles.astype(np.float32)[None]
        steps = cs.op_steps(op)
        return rng.uniform(-180.0, 180.0, size=(steps, len(sample), 4)).astype(np.float32)

    head, groups = cs.generate(0, n, oracle=True)
    worst = 0.0
    for it in head:
        fo.item(it)
    for g in groups:
        for it in g.pre:
            fo.item(it)
        fo.op(g, stand_in)
        worst = max(worst, fo.guarded.mean())
        for it in g.trail:
            fo.item(it)
        worst = max(worst, fo.guarded.mean())
    assert 0.0 < worst < CAP, worst
    # targets were picked and envs finished: the re-arms of the sequence are real ones
    assert fo.rearmed > len(sample) // 10
    # ... and neither appearance of the staged op runs on held envs only
    print(f"n = {n}: worst guarded share {worst:.4f}, re-armed {fo.rearmed}, reaching {reaching}")
    assert len(reaching) == 2 and min(reaching) >= cs.REACH_FLOOR, reaching


# ---- the alphabet covers the handle's entry points ---------------------------------------------------------------------
# method of StepEngine -> the ops of the alphabet (or items of a sequence) that call it
EXERCISED = {
    "reset": ("reset(points)",), "reset_random": ("reset_random",), "env_reset": ("env_reset(points)", "env_reset(None)"),
    "reset_done": ("reset_done",), "set_actions": ("set_actions(device)+step",), "sample_actions": ("sample_actions+step",),
    "step": ("step(host actions)", "set_actions(device)+step", "sample_actions+step", "ik(stage)+step"),
    "step_host": ("step_host",), "env_step": ("env_step",), "bad_action_count": ("bad_action_count",),
    "step_random": ("step_random",), "rollout": ("rollout",),
    "rollout_fused": ("rollout_fused(auto_reset=True)", "rollout_fused(auto_reset=False)"),
    "rollout_actions": ("rollout_actions", "rollout_actions(auto_reset=True)", "rollout_actions(dry_run=True)"),
    "rollout_policy": ("rollout_policy", "rollout_policy(auto_reset=True)"),
    "sample_population": ("sample_population",), "rollout_population": ("rollout_population",), "es": ("es",),
    "reward_to_go": ("reward_to_go",), "policy_grad": ("policy_grad",), "policy_eval": ("policy_eval",), "values": ("gae",),
    "gae": ("gae",), "value_grad": ("value_grad",), "shoot": ("shoot(commit=H)", "shoot(commit=0)"),
    "sample_plans": ("sample_plans",), "cem": ("cem(commit=H)", "cem(commit=0)"), "mppi": ("mppi(commit=H)", "mppi(commit=0)"),
    "jacobian": ("jacobian",), "ik": ("ik", "ik(stage)+step"), "observe": ("observe",), "check_done": ("check_done",),
    "get": ("get",), "set": ("set(F_GOALS)", "set(F_POINTS)", "set(F_ALIVE)"), "get_state": ("save_state",),
    "set_state": ("set_state",), "sync": ("sync",), "lap_begin": ("lap_begin+lap_end",), "lap_end": ("lap_begin+lap_end",),
    "dispatch": ("dispatch",), "return_stats": ("return_stats",), "gather_begin": ("gather_begin+gather_wait",),
    "gather_wait": ("gather_begin+gather_wait",), "gather_returns": ("gather_returns",),
}
# method -> why no op calls it
EXEMPT = {
    "close": "ends the handle: every sequence closes both of its handles when it is over",
    "step_kernel_name": "a name read from the handle, no device work; dispatch(), which is an op, reports the same schedule",
    "set_stream": "stream selection: a sequence stays on the stream its handle was created with",
    "use_torch_stream": "stream selection: the chains_torch regime calls it once, ahead of its sequence",
    "timer_start": "timer: brackets a region and must be paired; lap_begin+lap_end is the timers' op",
    "timer_stop": "timer: see timer_start",
    "timer_stop_async": "timer: see timer_start",
    "timer_read": "timer: see timer_start",
    "laps_total": "timer: reads and clears the laps' host-side list, no device state",
    "lap_times": "timer: see laps_total",
    "policy_size": "arithmetic on the handle's shape, no device work",
    "value_size": "arithmetic on the handle's shape, no device work",
    "flatten_policy": "a torch concatenation, no library call",
    "unflatten_policy": "views of a caller's tensor, no library call",
    "unflatten_value": "views of a caller's tensor, no library call",
    "device_ptr": "view: ends the records for good, which is how the twin is made (twin_of); tests/test_gpu_view_writes.py",
    "device_tensor": "view: device_ptr as a torch tensor; tests/test_gpu_view_writes.py",
    "ld": "view: the row stride, a device_ptr call",
    "goals": "get(F_GOALS); get is an op", "points": "get(F_POINTS); get is an op", "alives": "get(F_ALIVE); get is an op",
    "obs": "get(F_OBS); get is an op", "reward": "get(F_REWARD); get is an op", "done": "get(F_DONE); get is an op",
    "ground_hit": "get(F_REWARD) == -1; get is an op", "done_bits": "get(F_DONE_BITS); get is an op", "ee": "get(F_EE); get is an op",
    "total_reward": "get(F_TOTAL_REWARD); get is an op", "joints_coordinates": "get(F_JOINTS); get is an op",
    "episodes": "get(F_EPISODES); get is an op", "last_return": "get(F_LAST_RETURN); get is an op",
    "actions": "get(F_ACTIONS); get is an op", "return_ring": "get(F_RETURN_RING); get is an op",
    "finished": "get(F_EPISODES) minus the reset's index; get is an op", "zmin": "get(F_ZMIN); the snapshots read that field",
    "trace": "get(F_TRACE): needs a handle created with trace=True, which changes the step kernels",
    "comm_init": "constructor of a communicator: needs a second rank; tests/test_gpu_multirank_fake.py",
    "comm_destroy": "see comm_init",
    "total_envs": "n_envs without a communicator; gather_begin and gather_returns, which are ops, call it",
}


def test_every_public_method_of_the_handle_is_an_op_or_exempt():
    """A new entry point of StepEngine forces a decision: an op of the alphabet exercises it, or EXEMPT says why none does."""
    from manytor_amd.engine import StepEngine     # (imports without a GPU: tests/test_host_api.py)
    public = {name for name, v in vars(StepEngine).items()
              if not name.startswith("_") and (callable(v) or isinstance(v, (staticmethod, classmethod, property)))}
    assert {"ik", "jacobian", "step", "close"} <= public
    neither = sorted(public - set(EXERCISED) - set(EXEMPT))
    assert not neither, f"no op of tests/call_sequences.py calls {neither}: add one (or an exemption with its reason)"
    assert not set(EXERCISED) & set(EXEMPT)
    gone = sorted((set(EXERCISED) | set(EXEMPT)) - public)
    assert not gone, f"{gone}: no such method of StepEngine"
    items = {"reset_random", "rollout", "step_random", "save_state"}
    known = set(cs.alphabet(70144)) | items
    for method, ops in EXERCISED.items():
        assert ops and set(ops) <= known, (method, ops)
    assert all(reason.strip() for reason in EXEMPT.values())
