"""What mt_rollout_tape, mt_shoot, mt_cem and mt_mppi share on the host, pinned on all four at once: the refusal of a handle
the rollout kernels do not implement (the whole message, reason by reason, and the order of the reasons), the refusal
before a reset, and the commit every one of them ends in.

Shapes: n = 65 (one full 64-env block of the planners' grids plus a one-lane tail), one target, T = C = E = 1, the
reference table.  Nothing here depends on size; the planner tests hold the same properties at their own shapes.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_tape import EVERYTHING, SEED, assert_same, make_engine, snapshot

pytestmark = pytest.mark.gpu

N, K, T, D, TOL = 65, 1, 1, 4, 45.0
COMMIT_SEED = 0xC0FFEE
ENTRIES = ("mt_rollout_tape", "mt_shoot", "mt_cem", "mt_mppi")

# StepEngine keywords -> the reason as engine.hip spells it, in the order it tests them
REASONS = [
    ("frames", dict(obs_frame=1, ee_frame=-2), "custom obs_frame / ee_frame"),
    ("trace", dict(trace=True), "MT_FLAG_TRACE"),
    ("dh_in_lds", dict(dh_in_lds=True), "MT_FLAG_DH_IN_LDS"),
    ("hw_trig", dict(hw_trig=True), "MT_FLAG_HW_TRIG"),
    ("direct_trig", dict(direct_trig=True), "MT_FLAG_DIRECT_TRIG"),
    ("substeps27", dict(substeps=27), "substeps beyond the recurrence's reach (per-pose trigonometry)"),
    ("ablate", dict(ablate=1), "a profiling flag (MT_FLAG_ABLATE_*)"),
    ("trace+hw_trig", dict(trace=True, hw_trig=True), "MT_FLAG_TRACE"),         # two reasons at once: the earlier one
]


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def raw_call(eng, entry):
    """(rc, message) of the smallest well-formed evaluation; the rows stay NULL: each call here is refused ahead of them."""
    from manytor_amd import _lib as L
    arg = {"mt_rollout_tape": L.MtTape, "mt_shoot": L.MtShoot, "mt_cem": L.MtCem, "mt_mppi": L.MtMppi}[entry]()
    arg.struct_size, arg.n_steps, arg.ld = C.sizeof(arg), T, N
    if entry != "mt_rollout_tape":
        arg.n_candidates = 1
    if entry == "mt_shoot":
        arg.cand_stride = T * D * N
    if entry in ("mt_cem", "mt_mppi"):
        arg.lo, arg.hi = -180.0, 180.0
    if entry == "mt_cem":
        arg.n_elites = 1
    if entry == "mt_mppi":
        arg.decay = 0.5
    rc = getattr(eng._lib, entry)(eng._h, C.byref(arg))
    return rc, eng._lib.mt_last_error(eng._h).decode()


@pytest.mark.parametrize("kw,reason", [r[1:] for r in REASONS], ids=[r[0] for r in REASONS])
def test_every_entry_point_names_the_same_reason(m, kw, reason):
    eng = make_engine(m, "ref", N, K, TOL, **kw)
    eng.reset_random(SEED, 0)
    for entry in ENTRIES:
        rc, msg = raw_call(eng, entry)
        assert rc == m.lib.MT_ERR_UNSUPPORTED, (entry, rc, msg)
        assert msg == f"{entry}: not available on a handle with {reason}", (entry, msg)
    eng.close()


def test_every_entry_point_waits_for_a_reset(m):
    eng = make_engine(m, "ref", N, K, TOL)
    for entry in ENTRIES:
        rc, msg = raw_call(eng, entry)
        assert rc == m.lib.MT_ERR_STATE, (entry, rc, msg)
        assert msg == f"{entry} before mt_reset / mt_reset_random", (entry, msg)
    eng.close()


def moments(eng):
    import torch
    rng = np.random.RandomState(SEED)
    dev = torch.device("cuda", eng.device)
    mean = torch.from_numpy(rng.uniform(-180, 180, (T, D, N)).astype(np.float32)).to(dev)
    return mean, torch.full((T, D, N), 20.0, dtype=torch.float32, device=dev)


def committed(eng, planner):
    """One committed call of `planner`: (its result, the (1, D, N) tape it committed)."""
    import torch
    mean, sigma = moments(eng)
    kw = dict(commit=1, auto_reset=True, seed=COMMIT_SEED, returns=True)
    if planner == "shoot":
        plans = mean[None].contiguous()                                          # (C = 1, T, D, N)
        res = eng.shoot(plans, **kw)
        env = torch.arange(N, device=plans.device)
        return res, plans[res["best"].long(), :, :, env].permute(1, 2, 0)[:1].contiguous()       # each env's best plan
    if planner == "cem":
        res = eng.cem(mean, sigma, candidates=1, elites=1, **kw)
    else:
        res = eng.mppi(mean, sigma, candidates=1, decay=0.5, **kw)
    return res, res["chosen"][:1]


@pytest.mark.parametrize("planner", ["shoot", "cem", "mppi"])
def test_a_commit_is_the_tape_call_on_the_chosen_plan(m, planner):
    eng, twin = (make_engine(m, "ref", N, K, TOL) for _ in range(2))
    for e in (eng, twin):
        e.reset_random(SEED, 0)
    version = eng.version
    res, chosen = committed(eng, planner)
    assert eng.version == version + 1
    want = twin.rollout_actions(chosen, layout="soa", auto_reset=True, seed=COMMIT_SEED, returns=True)
    got = snapshot(m, eng, EVERYTHING)
    print(f"[commit-parity] {planner}: envs re-armed by the committed step {int((got['F_EPISODES'] > 0).sum())} of {N}")
    assert_same(got, snapshot(m, twin, EVERYTHING), f"{planner} commit vs rollout_actions")
    np.testing.assert_array_equal(res["returns"].cpu().numpy().view(np.uint32), want["returns"].cpu().numpy().view(np.uint32))
    eng.close()
    twin.close()
