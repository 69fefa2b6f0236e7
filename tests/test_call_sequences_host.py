"""CPU checks of tests/call_sequences.py, ahead of anything that needs a GPU: the generated sequences hold every op of the
alphabet in both positions, no stretch between two full resets is longer than MAX_STEPS env-steps, and the oracle leg's
sequences, played by the fp64 oracle alone, keep the share of envs that entered the guard band under the cap the GPU test
asserts at every comparison point (random fractional actions stand in for the policies' and the planners')."""
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

    def stand_in(op):
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
