"""mt_shoot / StepEngine.shoot: C candidate tapes per env scored from one state, the best named on the device, its first H
steps committed -- in one call.

Held to:
  * the calls it replaces: candidate_returns[c] == rollout_actions(plans[c], dry_run=True, returns=True) bit for bit, best ==
    numpy's argmax of those, and a commit == rollout_actions(the host-gathered best plans[:H]) on a twin handle, every field;
  * the fp64 C restatement of the reference (oracle/manytor_oracle.c) for every candidate of every env whose decision margins
    stay outside GUARD (tests/test_gpu_tape.py: same rule).

Inputs unless a test says otherwise: reset_random(SEED, 0); plans drawn uniformly in +-180 degrees with joints 1 and 2 scaled
by 0.4 (the planning example's shaping: returns spread over -T .. +K); two history steps drawn the same way and committed
first, so that the start state has dead targets, a non-zero return and stale outputs.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from parity_util import GUARD
from test_gpu_tape import EVERYTHING, SEED, _table, assert_same, make_engine, snapshot, unusable

pytestmark = pytest.mark.gpu

SHAPE = np.float32(0.4)


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


@functools.lru_cache(maxsize=None)
def shaped_plans(C_, T, n, D):
    """(plans (C, T, n, D), history (2, n, D)), float32, read-only."""
    rng = np.random.RandomState(SEED + T + n + C_)
    plans = rng.uniform(-180, 180, (C_, T, n, D)).astype(np.float32)
    plans[..., 1:3] *= SHAPE
    hist = rng.uniform(-180, 180, (2, n, D)).astype(np.float32)
    hist[..., 1:3] *= SHAPE
    plans.setflags(write=False)
    hist.setflags(write=False)
    return plans, hist


@functools.lru_cache(maxsize=None)
def turns_plans(C_, T, n, D):
    """test_gpu_tape.turns_tape's recipe per candidate: small angles plus whole turns out to +-32 400 degrees."""
    rng = np.random.RandomState(SEED + T + n + C_)
    small = rng.uniform(-60, 60, (C_, T, n, D))
    turns = rng.randint(-90, 91, (C_, 1, n, D))
    plans = (small + 360.0 * turns).astype(np.float32)
    hist = rng.uniform(-180, 180, (2, n, D)).astype(np.float32)
    hist[..., 1:3] *= SHAPE
    plans.setflags(write=False)
    hist.setflags(write=False)
    return plans, hist


def soa(plans):
    """(C, T, n, D) -> contiguous (C, T, D, n)"""
    return np.ascontiguousarray(plans.transpose(0, 1, 3, 2))


def started(m, table_name, n, k, tol, hist, **kw):
    eng = make_engine(m, table_name, n, k, tol, **kw)
    eng.reset_random(SEED, 0)
    eng.rollout_actions(hist)
    eng.sync()
    return eng


def dry_runs(eng, plans):
    """(C, n) float32: the return of every candidate through the call mt_shoot's evaluation is defined by."""
    rows = [eng.rollout_actions(plans[c], dry_run=True, returns=True)["returns"].cpu().numpy() for c in range(plans.shape[0])]
    return np.stack(rows)


def host(res):
    return {key: v.cpu().numpy() for key, v in res.items()}


# ---- 1. evaluation == C dry runs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("table_name,n,k,T,C_,tol,kind", [
    ("ref", 3001, 7, 8, 6, 20.0, "shaped"),       # n % 64 != 0, C % 4 != 0
    ("dh7", 5003, 3, 6, 5, 45.0, "shaped"),
    ("rt5", 1501, 3, 5, 3, 8.0, "shaped"),        # C < 4: a wave without candidates
    ("ref", 777, 32, 4, 2, 30.0, "shaped"),       # K = 32: the largest target tile
    ("ref", 1501, 3, 5, 9, 20.0, "shaped"),       # three candidates on one wave
    ("ref", 3001, 7, 8, 1, 20.0, "shaped"),
    ("ref", 300007, 7, 4, 2, 20.0, "shaped"),     # a two-chain handle, chains folded by the call's entry
    ("ref", 3001, 7, 6, 5, 8.0, "turns"),         # |angle| > 30 000 in every candidate: the wide form, taken per wave
])
def test_evaluation_equals_the_dry_runs_bit_for_bit(m, table_name, n, k, T, C_, tol, kind):
    D = len(_table(m, table_name)[0])
    plans, hist = (shaped_plans if kind == "shaped" else turns_plans)(C_, T, n, D)
    if kind == "turns":
        assert (np.abs(plans).reshape(C_, -1).max(axis=1) > 30000).all()
    eng = started(m, table_name, n, k, tol, hist)
    want = dry_runs(eng, plans)
    res = host(eng.shoot(soa(plans), all_returns=True))
    got = res["candidate_returns"]
    assert got.dtype == np.float32 and got.shape == (C_, n) and res["best"].dtype == np.int32
    differ = (want.max(axis=0) != want.min(axis=0)).mean()
    tied_top = ((want == want.max(axis=0)).sum(axis=0) > 1).mean()
    print(f"[shoot-vs-dry-runs] {table_name} n={n} K={k} T={T} C={C_} tol={tol} {kind}: envs whose candidates differ "
          f"{differ:.3f}, envs with a tied maximum {tied_top:.3f}, mean best return {want.max(axis=0).mean():+.3f}")
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(res["best"], np.argmax(want, axis=0))
    np.testing.assert_array_equal(res["best_return"], want.max(axis=0))
    if C_ > 1:      # (one candidate always "ties" with itself and never shares its maximum)
        assert differ > 0.5 and tied_top > 0.05, (differ, tied_top)
    # the env_major front end copies into the same layout
    res2 = host(eng.shoot(plans, layout="env_major"))
    np.testing.assert_array_equal(res2["best"], res["best"])
    assert "candidate_returns" not in res2
    eng.close()


# ---- 2. an evaluation changes nothing resident -------------------------------------------------------------------------
def test_evaluate_only_changes_nothing_resident(m):
    n, k, T, C_, tol = 3001, 7, 8, 6, 20.0
    plans, hist = shaped_plans(C_, T, n, 4)
    planted = plans.copy()
    planted[2, 1, 7, 0] = np.nan
    eng = started(m, "ref", n, k, tol, hist)
    eng.set_actions(hist[1] + np.float32(0.5))                     # an action row that no call below would write
    before = snapshot(m, eng, EVERYTHING)
    bad_before, version = eng.bad_action_count(), eng.version
    res = host(eng.shoot(soa(planted), all_returns=True))
    eng.sync()
    assert_same(snapshot(m, eng, EVERYTHING), before, "after the evaluation")
    assert eng.bad_action_count() == bad_before and eng.version == version
    np.testing.assert_array_equal(res["candidate_returns"], dry_runs(eng, planted))     # the held pose scores as the dry run's
    assert_same(snapshot(m, eng, EVERYTHING), before, "after the dry runs")
    eng.close()


# ---- 3. commit == the gathered tape on a twin handle -------------------------------------------------------------------
# `rearmed`: the number of envs that must have finished at least once in the committed steps (see the comment in the test).
@pytest.mark.parametrize("table_name,n,k,T,C_,H,tol,auto_reset,rearmed", [
    ("ref", 3001, 7, 8, 6, 3, 20.0, False, 0),
    ("ref", 3001, 7, 8, 6, 3, 20.0, True, 13),
    ("dh7", 5003, 3, 6, 5, 6, 45.0, True, 1000),      # H = T
    ("rt5", 1501, 3, 5, 3, 1, 8.0, False, 0),
])
def test_commit_equals_the_gathered_tape(m, table_name, n, k, T, C_, H, tol, auto_reset, rearmed):
    D = len(_table(m, table_name)[0])
    shaped, hist = shaped_plans(C_, T, n, D)
    plans = shaped.copy()
    rng = np.random.RandomState(SEED + 3)
    for c in range(C_):                                            # refused actions in every plane, also in the committed steps
        plans[c, 0, 11, 0] = np.nan                                # env 11, step 0: counted whichever plane wins
        for t in range(T):
            plans[c, t, rng.randint(0, n, 25), rng.randint(0, D)] = (np.nan, np.inf, -np.inf, np.float32(4e4))[(c + t) % 4]
    a = started(m, table_name, n, k, tol, hist)
    b = started(m, table_name, n, k, tol, hist)
    got = host(a.shoot(soa(plans), commit=H, auto_reset=auto_reset, seed=SEED, all_returns=True, log=True, returns=True))
    a.sync()

    scores = dry_runs(b, plans)
    best = np.argmax(scores, axis=0)
    chosen = np.ascontiguousarray(plans[best, :, np.arange(n), :].transpose(1, 0, 2))      # (T, n, D)
    want = host(b.rollout_actions(chosen[:H], auto_reset=auto_reset, seed=SEED, log=True, returns=True))
    b.sync()
    held = sum(int(unusable(chosen[t]).sum()) for t in range(H))
    finished = int((a.finished() > 0).sum())
    print(f"[shoot-commit] {table_name} n={n} K={k} T={T} C={C_} H={H} auto_reset={auto_reset}: held pairs {held}, "
          f"envs re-armed {finished}")

    np.testing.assert_array_equal(got["candidate_returns"], scores)
    np.testing.assert_array_equal(got["best"], best)
    assert_same(snapshot(m, a, EVERYTHING), snapshot(m, b, EVERYTHING), "shoot(commit) vs the gathered tape")
    for key in ("reward", "done", "returns"):
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert held >= 1 and a.bad_action_count() == held == b.bad_action_count()
    assert a.version == b.version
    if auto_reset:
        # The fp64 oracle alone finishes 813 (ref) and 3 637 (dh7) envs under SOME candidate of these inputs within T steps.
        # Within the H COMMITTED steps of the plans it chooses itself (these planted inputs) it finishes 27 (ref, H = 3 of
        # T = 8) and 3 344 (dh7, H = T) envs: 50 is out of reach for the ref case, its floor is half the oracle's figure, 13.
        assert finished > rearmed, "the re-arm path was not exercised"
    a.close()
    b.close()


# ---- 4. against the fp64 oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("table_name,n,k,T,C_,tol", [
    ("ref", 3001, 7, 8, 6, 20.0),
    ("dh7", 5003, 3, 6, 5, 45.0),
])
def test_every_candidate_against_the_c_oracle(m, table_name, n, k, T, C_, tol):
    from oracle import c_oracle
    table, radius = _table(m, table_name)
    D = len(table)
    plans, hist = shaped_plans(C_, T, n, D)
    eng = started(m, table_name, n, k, tol, hist)
    goals, points, alive = eng.goals().astype(np.float64), eng.points().astype(np.float64), eng.alives()
    ora = c_oracle.COracle(n, k, table=np.asarray(table), substeps=25, radius=radius, pickup_tol=tol, threads=16)
    clean = np.ones(n, dtype=bool)
    want = np.zeros((C_, n))
    for c in range(C_):
        ora.reset(points)                                          # every candidate starts from the engine's state
        ora.goals[:] = goals
        ora.alive_u8[:] = alive
        for t in range(T):
            pre_alive = ora.alives.copy()
            _, rew, _ = ora.step(plans[c, t].astype(np.float64))
            pm = np.where(pre_alive, ora.pickup_margin, np.inf).min(axis=1)
            clean &= ~((ora.ground_margin < GUARD) | (pm < GUARD))
            want[c] += rew
    res = host(eng.shoot(soa(plans), all_returns=True))
    print(f"[shoot-vs-oracle] {table_name} n={n} K={k} T={T} C={C_} tol={tol}: clean share {clean.mean():.4f}")
    assert clean.mean() >= 0.90, clean.mean()
    np.testing.assert_array_equal(res["candidate_returns"][:, clean], want[:, clean].astype(np.float32))
    np.testing.assert_array_equal(res["best"][clean], np.argmax(want, axis=0)[clean])
    np.testing.assert_array_equal(res["best_return"][clean], want.max(axis=0)[clean].astype(np.float32))
    eng.close()


# ---- 5. the tie rule ---------------------------------------------------------------------------------------------------
def test_a_tie_goes_to_the_lowest_index(m):
    n, k, T, C_, tol = 3001, 7, 8, 6, 20.0
    shaped, hist = shaped_plans(C_, T, n, 4)
    plans = np.full_like(shaped, np.nan)                           # an all-NaN plane holds the pose throughout
    plans[0] = plans[1] = plans[3] = shaped[0]
    eng = started(m, "ref", n, k, tol, hist)
    res = host(eng.shoot(soa(plans), all_returns=True))
    cand = res["candidate_returns"]
    np.testing.assert_array_equal(cand[1], cand[0])
    np.testing.assert_array_equal(cand[3], cand[0])
    assert (cand[[2, 4, 5]] <= 0).all()                            # a held pose picks nothing up
    first = res["best_return"] == cand[0]
    print(f"[shoot-ties] plane 0 earns > 0 in {(cand[0] > 0).sum()} of {n} envs")
    assert (res["best"][first] == 0).all() and (cand[0] > 0).any() and first[cand[0] > 0].all()
    assert not np.isin(res["best"], (1, 3)).any()
    np.testing.assert_array_equal(res["best"], np.argmax(cand, axis=0))
    eng.close()


# ---- 6. pitches through the C entry point ------------------------------------------------------------------------------
def test_pitches_through_the_c_entry_point(m):
    import torch
    L = m.lib
    n, k, T, C_, H, tol, D = 3001, 7, 8, 6, 2, 20.0, 4
    ld, ret_ld, log_ld = n + 37, n + 5, n + 3
    stride = T * D * ld + 1000
    plans, hist = shaped_plans(C_, T, n, D)
    dense = started(m, "ref", n, k, tol, hist)
    want = host(dense.shoot(soa(plans), commit=H, seed=SEED, all_returns=True, log=True, returns=True))
    dense.sync()

    eng = started(m, "ref", n, k, tol, hist)
    dev = torch.device("cuda", eng.device)
    nan = float("nan")
    buf = torch.full((C_ * stride,), nan, dtype=torch.float32, device=dev)               # pads are never read
    src = torch.from_numpy(soa(plans)).to(dev)
    for c in range(C_):
        buf[c * stride:c * stride + T * D * ld].view(T * D, ld)[:, :n] = src[c].reshape(T * D, n)
    rets = torch.full((C_, ret_ld), nan, dtype=torch.float32, device=dev)
    best = torch.full((n,), -1, dtype=torch.int32, device=dev)
    best_ret = torch.full((n,), nan, dtype=torch.float32, device=dev)
    rew = torch.full((H, log_ld), 0x55, dtype=torch.int8, device=dev)
    done = torch.full((H, log_ld), 0xAA, dtype=torch.uint8, device=dev)
    ret = torch.full((n,), nan, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    arg = L.MtShoot()
    arg.struct_size, arg.n_steps, arg.n_candidates, arg.commit_steps = C.sizeof(L.MtShoot), T, C_, H
    arg.actions, arg.ld, arg.cand_stride = buf.data_ptr(), ld, stride
    arg.returns_out, arg.ret_ld, arg.best_out, arg.best_return_out = rets.data_ptr(), ret_ld, best.data_ptr(), best_ret.data_ptr()
    arg.reward_log, arg.done_log, arg.log_ld, arg.return_out = rew.data_ptr(), done.data_ptr(), log_ld, ret.data_ptr()
    arg.seed, arg.flags = SEED, 0
    assert eng._lib.mt_shoot(eng._h, C.byref(arg)) == L.MT_OK, eng._lib.mt_last_error(eng._h)
    eng.sync()
    rets, rew, done = rets.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
    np.testing.assert_array_equal(rets[:, :n], want["candidate_returns"])
    assert np.isnan(rets[:, n:]).all() and (rew[:, n:] == 0x55).all() and (done[:, n:] == 0xAA).all()
    np.testing.assert_array_equal(best.cpu().numpy(), want["best"])
    np.testing.assert_array_equal(best_ret.cpu().numpy(), want["best_return"])
    np.testing.assert_array_equal(rew[:, :n], want["reward"])
    np.testing.assert_array_equal(done[:, :n], want["done"])
    np.testing.assert_array_equal(ret.cpu().numpy(), want["returns"])
    assert_same(snapshot(m, eng, EVERYTHING), snapshot(m, dense, EVERYTHING), "pitched vs dense")
    # the same pitches through the Python front end: a (C, T, D, N) view of the padded block goes in zero-copy
    view = torch.as_strided(buf, (C_, T, D, n), (stride, D * ld, ld, 1))
    made, made_ld, made_stride = eng._tape_tensor(view, "soa", candidates=True)
    assert made.data_ptr() == buf.data_ptr() and (made_ld, made_stride) == (ld, stride)
    again = host(eng.shoot(view, all_returns=True))
    np.testing.assert_array_equal(again["candidate_returns"], dry_runs(eng, plans))
    strided = torch.zeros((C_, T, D, 2 * n), dtype=torch.float32, device=dev)[..., ::2]  # env stride 2: made contiguous
    made, made_ld, made_stride = eng._tape_tensor(strided, "soa", candidates=True)
    assert made.is_contiguous() and (made_ld, made_stride) == (n, T * D * n) and made.data_ptr() != strided.data_ptr()
    eng.close()
    dense.close()


# ---- 7. errors -----------------------------------------------------------------------------------------------------------
def test_error_returns_and_dispatch_entry(m):
    import torch
    L = m.lib
    n, T, D, C_ = 3001, 3, 4, 2
    eng = make_engine(m, "ref", n, 7, 8.0)
    dev = torch.device("cuda", eng.device)
    plans = torch.zeros((C_ * T * D, n), dtype=torch.float32, device=dev)
    best = torch.zeros((n,), dtype=torch.int32, device=dev)
    rets = torch.zeros((C_, n), dtype=torch.float32, device=dev)
    logs = torch.zeros((T, n), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)

    def call(engine=eng, **over):
        arg = L.MtShoot()
        arg.struct_size, arg.n_steps, arg.n_candidates, arg.commit_steps = C.sizeof(L.MtShoot), T, C_, 0
        arg.actions, arg.ld, arg.cand_stride, arg.best_out = plans.data_ptr(), n, T * D * n, best.data_ptr()
        for key, v in over.items():
            setattr(arg, key, v)
        rc = engine._lib.mt_shoot(engine._h, C.byref(arg))
        return rc, engine._lib.mt_last_error(engine._h).decode()

    rc, msg = call()
    assert rc == L.MT_ERR_STATE and "reset" in msg                              # before a reset
    eng.reset_random(SEED, 0)
    assert call()[0] == L.MT_OK
    assert call(best_out=None)[0] == L.MT_OK                                    # an evaluation may go without it
    assert call(commit_steps=T, log_ld=0)[0] == L.MT_OK                         # no log given: the pitch is not looked at
    eng.sync()
    before = snapshot(m, eng, EVERYTHING)
    for over, field in ((dict(struct_size=C.sizeof(L.MtShoot) - 8), "struct_size"),
                        (dict(reserved=1), "reserved"),
                        (dict(flags=0x2), "flags"),
                        (dict(n_steps=-1), "n_steps"),
                        (dict(n_candidates=0), "n_candidates"),
                        (dict(n_candidates=65), "n_candidates"),
                        (dict(commit_steps=-1), "commit_steps"),
                        (dict(commit_steps=T + 1), "commit_steps"),
                        (dict(flags=L.SHOOT_AUTO_RESET), "commit_steps"),      # AUTO_RESET with H = 0
                        (dict(commit_steps=1, best_out=None), "best_out"),
                        (dict(actions=None), "actions"),
                        (dict(ld=n - 1), "ld"),
                        (dict(cand_stride=T * D * n - 1), "cand_stride"),
                        (dict(returns_out=rets.data_ptr(), ret_ld=n - 1), "ret_ld"),
                        (dict(commit_steps=1, reward_log=logs.data_ptr(), log_ld=n - 1), "log_ld"),
                        (dict(commit_steps=1, done_log=logs.data_ptr(), log_ld=0), "log_ld")):
        rc, msg = call(**over)
        assert rc == L.MT_ERR_INVALID_ARG and field in msg, (over, rc, msg)
    assert call(n_steps=0, actions=None)[0] == L.MT_OK                          # T = 0: a no-op
    eng.sync()
    assert_same(snapshot(m, eng, EVERYTHING), before, "after the refused calls and T = 0")
    version = eng.version
    res = eng.shoot(np.zeros((C_, 0, D, n), dtype=np.float32))
    assert res["best"].shape == (n,) and eng.version == version
    with pytest.raises(ValueError):
        eng.shoot(np.zeros((65, 1, D, n), dtype=np.float32))
    with pytest.raises(ValueError):
        eng.shoot(np.zeros((C_, T, D, n), dtype=np.float32), commit=T + 1)

    tr = make_engine(m, "ref", n, 7, 8.0, trace=True)
    tr.reset_random(SEED, 0)
    rc, msg = call(engine=tr)
    assert rc == L.MT_ERR_UNSUPPORTED and "mt_shoot: not available on a handle with MT_FLAG_TRACE" in msg
    with pytest.raises(m.ManytorError):
        tr.shoot(np.zeros((C_, T, D, n), dtype=np.float32))
    assert tr.dispatch()["shoot"]["usable"] is False
    d = eng.dispatch()["shoot"]
    assert d == {"usable": True, "envs_per_block": 64, "waves_per_block": 4}
    tr.close()
    eng.close()


# ---- 8. stream order on a caller's stream ------------------------------------------------------------------------------
def test_shoot_is_ordered_with_torch_ops_on_the_callers_stream(m):
    import torch
    n, k, T, C_, H, tol = 3001, 7, 8, 6, 3, 20.0
    plans, hist = shaped_plans(C_, T, n, 4)
    block = soa(plans)
    own = started(m, "ref", n, k, tol, hist)
    want = host(own.shoot(block, commit=H, auto_reset=True, seed=SEED, returns=True))
    own.sync()

    eng = make_engine(m, "ref", n, k, tol)
    eng.use_torch_stream()
    eng.reset_random(SEED, 0)
    eng.rollout_actions(hist)
    dev = torch.device("cuda", eng.device)
    src = torch.from_numpy(block).to(dev)
    buf = torch.zeros_like(src)
    ballast = torch.ones((2048, 2048), device=dev)
    torch.cuda.synchronize(dev)
    for _ in range(8):                                             # keeps the stream busy ahead of the plans' writer
        ballast = ballast @ ballast * 1e-4
    buf.copy_(src)                                                 # the torch op that writes the plans ...
    res = eng.shoot(buf, commit=H, auto_reset=True, seed=SEED, returns=True)   # ... read in place, no host sync ...
    hist_best = torch.bincount(res["best"].to(torch.int64), minlength=C_)      # ... and a torch op on `best` right behind
    buf.zero_()                                                    # (a later write must not reach the call either)
    torch.cuda.synchronize(dev)
    np.testing.assert_array_equal(hist_best.cpu().numpy(), np.bincount(want["best"], minlength=C_))
    for key in ("best", "best_return", "returns"):
        np.testing.assert_array_equal(res[key].cpu().numpy(), want[key], err_msg=key)
    assert_same(snapshot(m, eng, EVERYTHING), snapshot(m, own, EVERYTHING), "caller's stream vs own stream")
    assert len(np.unique(want["best"])) == C_
    eng.close()
    own.close()


# ---- 9. stream capture -------------------------------------------------------------------------------------------------
def test_shoot_is_capturable_in_a_hip_graph(m):
    """One linear capture on one side stream records `static_plans.copy_(staging); mt_shoot(commit = H)` with preallocated
    outputs; each of two replays with fresh plans equals the eager call on a twin: outputs and the state behind them."""
    import torch
    L = m.lib
    n, k, T, C_, H, D, tol, replays = 3001, 7, 6, 5, 2, 4, 20.0, 2
    eager, graphed = make_engine(m, "ref", n, k, tol), make_engine(m, "ref", n, k, tol)
    for e in (eager, graphed):
        e.use_torch_stream()
        e.reset_random(SEED, 0)
    dev = torch.device("cuda", graphed.device)
    src = torch.stack([torch.from_numpy(soa(shaped_plans(C_, T, n + r, D)[0][:, :, :n])) for r in range(replays)]).to(dev)
    staging = torch.zeros((C_, T, D, n), dtype=torch.float32, device=dev)      # refreshed in front of every replay
    static_plans = torch.zeros_like(staging)
    best = torch.zeros((n,), dtype=torch.int32, device=dev)
    best_ret = torch.zeros((n,), dtype=torch.float32, device=dev)
    rew = torch.zeros((H, n), dtype=torch.int8, device=dev)
    done = torch.zeros((H, n), dtype=torch.uint8, device=dev)
    ret = torch.zeros((n,), dtype=torch.float32, device=dev)
    arg = L.MtShoot()
    arg.struct_size, arg.n_steps, arg.n_candidates, arg.commit_steps = C.sizeof(L.MtShoot), T, C_, H
    arg.actions, arg.ld, arg.cand_stride = static_plans.data_ptr(), n, T * D * n
    arg.best_out, arg.best_return_out = best.data_ptr(), best_ret.data_ptr()
    arg.reward_log, arg.done_log, arg.log_ld, arg.return_out = rew.data_ptr(), done.data_ptr(), n, ret.data_ptr()
    arg.seed, arg.flags = SEED, L.SHOOT_AUTO_RESET
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        graphed.use_torch_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static_plans.copy_(staging)
            rc = graphed._lib.mt_shoot(graphed._h, C.byref(arg))
    assert rc == L.MT_OK, graphed._lib.mt_last_error(graphed._h)
    torch.cuda.synchronize(dev)
    graphed.reset_random(SEED, 0)         # the capture pass itself does not execute; start from the same state anyway
    torch.cuda.synchronize(dev)
    for r in range(replays):
        want = host(eager.shoot(src[r], commit=H, auto_reset=True, seed=SEED, log=True, returns=True))
        staging.copy_(src[r])
        graph.replay()
        torch.cuda.synchronize(dev)
        for key, got in (("best", best), ("best_return", best_ret), ("reward", rew), ("done", done), ("returns", ret)):
            np.testing.assert_array_equal(got.cpu().numpy(), want[key], err_msg=f"replay {r} {key}")
        assert np.abs(want["reward"]).sum() > 0
        assert_same(snapshot(m, graphed, EVERYTHING), snapshot(m, eager, EVERYTHING), f"replay {r}")
    eager.close()
    graphed.close()
