"""mt_mppi / StepEngine.mppi: one MPPI iteration in one call, the candidates drawn in the kernel from mt_cem's stream.

Held to:
  * tests/mppi_ref.py, the numpy restatement of the table of powers, the gap, the weights and the refit (bit for bit; the
    hardware square root of sigma_out within 1 ulp), on the block tests/cem_ref.py restates;
  * the calls that already exist: the evaluation == shoot() on the block sample_plans() writes, a commit == rollout_actions(
    chosen) on a twin handle, every field;
  * the fp64 C restatement of the reference (oracle/manytor_oracle.c) for every candidate of every env whose decision
    margins stay outside GUARD (tests/test_gpu_shoot.py: same rule).

Inputs: tests/test_gpu_cem.py's -- the same handles, histories, means and sigmas, case by case.
"""
import ctypes as C

import numpy as np
import pytest

import mppi_ref
from parity_util import GUARD
from test_gpu_cem import CASES, PLAN_SEED, case_inputs, dev, history, shaped_moments, ulps
from test_gpu_shoot import dry_runs, host, started
from test_gpu_tape import EVERYTHING, SEED, _table, assert_same, make_engine, snapshot, unusable

pytestmark = pytest.mark.gpu

DECAYS = (0.25, float(mppi_ref.decay_of(1.5)), 0.9990234375)


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. evaluation == shoot() on the sampled block ----------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + [("ref", 300007, 7, 4, 2, 20.0, "shaped", 0, 5, False)],      # + a two-chain handle
                         ids=lambda c: f"{c[0]}-{c[1]}-C{c[4]}-{c[6]}-base{c[7]}")
def test_evaluation_equals_shoot_on_the_sampled_block(m, case):
    eng, mean, sigma, kw = case_inputs(m, case)
    C_, kind = case[4], case[6]
    mean_d, sigma_d = dev(eng, mean), dev(eng, sigma)
    block = eng.sample_plans(mean_d, sigma_d, **kw)
    if kind == "turns":
        assert (block.abs().reshape(C_, -1).max(dim=1).values > 30000).all()
    want = host(eng.shoot(block, all_returns=True))
    got = host(eng.mppi(mean_d, sigma_d, temperature=1.5, all_returns=True, **kw))
    differ = (want["candidate_returns"].max(axis=0) != want["candidate_returns"].min(axis=0)).mean()
    print(f"[mppi-vs-shoot] {case}: envs whose candidates differ {differ:.3f}, mean best return {want['best_return'].mean():+.3f}")
    assert got["candidate_returns"].dtype == np.float32 and got["best"].dtype == np.int32
    np.testing.assert_array_equal(got["candidate_returns"], want["candidate_returns"])
    np.testing.assert_array_equal(got["best"], want["best"])
    np.testing.assert_array_equal(got["best_return"], want["best_return"])
    assert differ > 0.05, differ
    eng.close()


# ---- 2. weights and refit == the restatement ----------------------------------------------------------------------------
# `mixed`: half of the share of envs with at least two distinct weights on these inputs, by the dry runs on the sampled block
# and the restatement alone (the scores below are asserted equal to the dry runs before the share is taken): 1.0000 (ref)
# and 0.8797 (dh7), the same at all three decays -- no power of these decays underflows within 2 T.  The floor shows that
# the weights really differ within an env.
@pytest.mark.parametrize("decay", DECAYS, ids=lambda d: f"decay{d:.4f}")
@pytest.mark.parametrize("table_name,n,k,T,C_,tol,sigma_min,keep,mixed", [
    ("ref", 3001, 7, 8, 6, 20.0, 0.5, False, 0.5),
    ("dh7", 5003, 3, 6, 5, 45.0, 30.0, True, 0.4398),
])
def test_weights_and_refit_equal_the_restatement(m, table_name, n, k, T, C_, tol, sigma_min, keep, mixed, decay):
    """weights against W[gap] on the returned scores (which equal the dry runs), weight_sum and mean_out bit for bit,
    sigma_out within 1 ulp (a hardware square root may be 1 ulp off) and exactly sigma_min under the floor."""
    D = len(_table(m, table_name)[0])
    mean, sigma = shaped_moments(T, n, D)
    eng = started(m, table_name, n, k, tol, history(C_, T, n, D))
    kw = dict(candidates=C_, draw=9, seed=PLAN_SEED, keep_mean=keep)
    mean_d, sigma_d = dev(eng, mean), dev(eng, sigma)
    block = eng.sample_plans(mean_d, sigma_d, **kw).cpu().numpy()
    got = host(eng.mppi(mean_d, sigma_d, decay=decay, sigma_min=sigma_min, fit_sigma=True, all_returns=True, weights=True, **kw))
    fixed = host(eng.mppi(mean_d, sigma_d, decay=decay, **kw))     # mean_out alone: a fixed-sigma MPPI
    scores = got["candidate_returns"]
    np.testing.assert_array_equal(scores, dry_runs(eng, block.transpose(0, 1, 3, 2)))
    want_w = mppi_ref.weights(scores, decay, T)
    share = float((want_w.max(axis=0) != want_w.min(axis=0)).mean())
    print(f"[mppi-weights] {table_name} n={n} C={C_} decay={decay!r}: envs with two distinct weights {share:.4f}, "
          f"smallest weight {want_w.min():.3e}")
    assert share >= mixed, (share, mixed)
    assert got["weights"].dtype == np.float32 and got["weights"].shape == (C_, n)
    np.testing.assert_array_equal(bits(got["weights"]), bits(want_w))
    np.testing.assert_array_equal(bits(got["weight_sum"]), bits(mppi_ref.weight_sum(want_w)))
    assert (got["weight_sum"] >= 1).all() and (got["weight_sum"] <= C_).all()
    want_m, want_s = mppi_ref.refit(block, want_w, sigma_min)
    np.testing.assert_array_equal(bits(got["mean"]), bits(want_m))
    assert "sigma" not in fixed
    np.testing.assert_array_equal(bits(fixed["mean"]), bits(want_m))
    np.testing.assert_array_equal(bits(fixed["weight_sum"]), bits(got["weight_sum"]))
    worst = int(ulps(got["sigma"], want_s).max())
    floored = want_s == np.float32(sigma_min)
    print(f"[mppi-refit] sigma_out: worst distance {worst} ulp, floored share {floored.mean():.4f}")
    assert worst <= 1, worst
    assert (got["sigma"] >= np.float32(sigma_min)).all()
    raw_s = mppi_ref.refit(block, want_w, 0.0)[1]
    clearly = raw_s * np.float32(1.000001) < np.float32(sigma_min)             # below the floor by more than an ulp
    np.testing.assert_array_equal(got["sigma"][clearly], np.float32(sigma_min))
    eng.close()


# ---- 3. limits ----------------------------------------------------------------------------------------------------------
def test_decay_zero_is_the_hard_maximum_and_decay_one_the_plain_average(m):
    n, k, T, C_, tol, sigma_min = 3001, 7, 8, 6, 20.0, 1.25
    mean, sigma = shaped_moments(T, n, 4)
    eng = started(m, "ref", n, k, tol, history(C_, T, n, 4))
    kw = dict(candidates=C_, draw=9, seed=PLAN_SEED, sigma_min=sigma_min, fit_sigma=True, all_returns=True, weights=True)
    mean_d, sigma_d = dev(eng, mean), dev(eng, sigma)
    block = eng.sample_plans(mean_d, sigma_d, candidates=C_, draw=9, seed=PLAN_SEED).cpu().numpy()

    hard = host(eng.mppi(mean_d, sigma_d, decay=0.0, **kw))
    scores = hard["candidate_returns"]
    tied = (scores == scores.max(axis=0)).sum(axis=0)
    assert np.isin(hard["weights"], (0.0, 1.0)).all()
    np.testing.assert_array_equal(hard["weights"], (scores == scores.max(axis=0)).astype(np.float32))
    np.testing.assert_array_equal(hard["weight_sum"], tied.astype(np.float32))
    unique = tied == 1
    print(f"[mppi-limits] decay 0: envs with a unique best {unique.mean():.4f}")
    assert 0.05 < unique.mean() < 1.0                              # both kinds of env are there
    picked = block[hard["best"], :, :, np.arange(n)].transpose(1, 2, 0)        # (T, D, n)
    np.testing.assert_array_equal(bits(hard["mean"][:, :, unique]), bits(picked[:, :, unique]))
    np.testing.assert_array_equal(hard["sigma"][:, :, unique], np.float32(sigma_min))
    want_m, want_s = mppi_ref.refit(block, hard["weights"], sigma_min)
    np.testing.assert_array_equal(bits(hard["mean"]), bits(want_m))
    assert int(ulps(hard["sigma"], want_s).max()) <= 1

    flat = host(eng.mppi(mean_d, sigma_d, decay=1.0, **kw))
    np.testing.assert_array_equal(flat["candidate_returns"], scores)
    np.testing.assert_array_equal(flat["weights"], np.float32(1))
    np.testing.assert_array_equal(flat["weight_sum"], np.float32(C_))
    want_m, want_s = mppi_ref.refit(block, np.ones((C_, n), dtype=np.float32), sigma_min)
    np.testing.assert_array_equal(bits(flat["mean"]), bits(want_m))
    assert int(ulps(flat["sigma"], want_s).max()) <= 1
    eng.close()


def test_sigma_zero_makes_every_candidate_the_mean(m):
    n, k, T, C_, tol = 3001, 7, 8, 6, 20.0
    mean, _ = shaped_moments(T, n, 4)
    eng = started(m, "ref", n, k, tol, history(C_, T, n, 4))
    mean_d = dev(eng, mean)
    got = host(eng.mppi(mean_d, mean_d * 0, candidates=C_, decay=0.25, sigma_min=1.25, seed=PLAN_SEED, fit_sigma=True,
                        all_returns=True, weights=True))
    scores = got["candidate_returns"]
    np.testing.assert_array_equal(scores, np.broadcast_to(scores[0], scores.shape))
    np.testing.assert_array_equal(scores[0], dry_runs(eng, mean.transpose(0, 2, 1)[None])[0])
    assert (got["best"] == 0).all()
    np.testing.assert_array_equal(got["weights"], np.float32(1))
    np.testing.assert_array_equal(got["weight_sum"], np.float32(C_))
    np.testing.assert_array_equal(got["sigma"], np.float32(1.25))
    np.testing.assert_allclose(got["mean"], mean, rtol=6e-7, atol=0)           # 6 x / 6: five sums and a division round
    eng.close()


# ---- 4. in place == out of place ----------------------------------------------------------------------------------------
def test_in_place_refit_equals_out_of_place(m):
    n, k, T, C_, H, tol = 3001, 7, 8, 6, 2, 20.0
    mean, sigma = shaped_moments(T, n, 4)
    a = started(m, "ref", n, k, tol, history(C_, T, n, 4))
    b = started(m, "ref", n, k, tol, history(C_, T, n, 4))
    c = started(m, "ref", n, k, tol, history(C_, T, n, 4))
    kw = dict(candidates=C_, temperature=1.5, seed=PLAN_SEED, draw=2, commit=H, sigma_min=0.5, all_returns=True, weights=True,
              keep_mean=True)
    mean_a, sigma_a, mean_b, sigma_b, mean_c, sigma_c = (dev(e, v) for e in (a, b, c) for v in (mean, sigma))
    out = a.mppi(mean_a, sigma_a, fit_sigma=True, **kw)
    inp = b.mppi(mean_b, sigma_b, fit_sigma=True, inplace=True, **kw)
    only = c.mppi(mean_c, sigma_c, inplace=True, **kw)             # the mean alone in place: sigma stays
    assert inp["mean"] is mean_b and inp["sigma"] is sigma_b and out["mean"] is not mean_a and only["mean"] is mean_c
    np.testing.assert_array_equal(mean_a.cpu().numpy(), mean)                  # out of place: the inputs stay
    np.testing.assert_array_equal(sigma_a.cpu().numpy(), sigma)
    np.testing.assert_array_equal(sigma_c.cpu().numpy(), sigma)
    out, inp, only = host(out), host(inp), host(only)
    assert (out["mean"] != mean).mean() > 0.9 and (out["sigma"] != sigma).mean() > 0.9
    for key in out:
        np.testing.assert_array_equal(inp[key], out[key], err_msg=key)
    for key in only:
        np.testing.assert_array_equal(only[key], out[key], err_msg=key)
    assert_same(snapshot(m, b, EVERYTHING), snapshot(m, a, EVERYTHING), "in place vs out of place")
    assert_same(snapshot(m, c, EVERYTHING), snapshot(m, a, EVERYTHING), "mean in place vs out of place")
    for e in (a, b, c):
        e.close()


# ---- 5. an evaluation changes nothing resident; a NaN stays in its env -------------------------------------------------
def test_evaluate_only_changes_nothing_resident_and_a_nan_stays_in_its_env(m):
    n, k, T, C_, tol, env = 3001, 7, 8, 6, 20.0, 1000
    mean, sigma = shaped_moments(T, n, 4)
    hist = history(C_, T, n, 4)
    eng = started(m, "ref", n, k, tol, hist)
    eng.set_actions(hist[1] + np.float32(0.5))                     # an action row that no call below would write
    before = snapshot(m, eng, EVERYTHING)
    bad_before, version = eng.bad_action_count(), eng.version
    kw = dict(candidates=C_, temperature=1.5, seed=PLAN_SEED, fit_sigma=True, all_returns=True, weights=True)
    clean = host(eng.mppi(dev(eng, mean), dev(eng, sigma), **kw))
    planted = mean.copy()
    planted[:, 2, env] = np.nan                                    # every step of one env: its candidates hold the pose
    got = host(eng.mppi(dev(eng, planted), dev(eng, sigma), **kw))
    eng.sync()
    assert_same(snapshot(m, eng, EVERYTHING), before, "after two evaluations")
    assert eng.bad_action_count() == bad_before and eng.version == version
    others = np.arange(n) != env
    for key in clean:
        np.testing.assert_array_equal(got[key][..., others], clean[key][..., others], err_msg=key)
    held = np.full((1, T, n, 4), np.nan, dtype=np.float32)
    np.testing.assert_array_equal(got["candidate_returns"][:, env], np.repeat(dry_runs(eng, held)[0, env], C_))
    assert got["best"][env] == 0 and got["weight_sum"][env] == C_ and (got["weights"][:, env] == 1).all()
    eng.close()


# ---- 6. commit == rollout_actions(chosen) on a twin handle -------------------------------------------------------------
# `rearmed`: the floors tests/test_gpu_cem.py records for the same inputs (the block and its best plans are the same)
@pytest.mark.parametrize("table_name,n,k,T,C_,H,tol,auto_reset,rearmed", [
    ("ref", 3001, 7, 8, 6, 3, 20.0, False, 0),
    ("ref", 3001, 7, 8, 6, 3, 20.0, True, 12),
    ("dh7", 5003, 3, 6, 5, 6, 45.0, True, 1498),                   # H = T
])
def test_commit_equals_the_chosen_tape_on_a_twin(m, table_name, n, k, T, C_, H, tol, auto_reset, rearmed):
    D = len(_table(m, table_name)[0])
    shaped, sigma = shaped_moments(T, n, D)
    mean = shaped.copy()
    mean[0, 0, 11] = np.nan                                        # env 11 holds its pose in step 0 whichever plan wins: counted
    mean[H - 1, D - 1, 64] = np.inf
    hist = history(C_, T, n, D)
    a = started(m, table_name, n, k, tol, hist)
    b = started(m, table_name, n, k, tol, hist)
    kw = dict(candidates=C_, draw=5, seed=PLAN_SEED)
    mean_d, sigma_d = dev(a, mean), dev(a, sigma)
    block = a.sample_plans(mean_d, sigma_d, **kw).cpu().numpy()
    got = a.mppi(mean_d, sigma_d, temperature=1.5, commit=H, auto_reset=auto_reset, log=True, returns=True, **kw)
    a.sync()
    chosen = got["chosen"]
    got = host(got)
    np.testing.assert_array_equal(bits(got["chosen"]), bits(block[got["best"], :H, :, np.arange(n)].transpose(1, 2, 0)))
    want = host(b.rollout_actions(chosen, layout="soa", auto_reset=auto_reset, seed=PLAN_SEED, log=True, returns=True))
    b.sync()
    held = sum(int(unusable(got["chosen"][t].T).sum()) for t in range(H))
    finished = int((b.finished() > 0).sum())
    print(f"[mppi-commit] {table_name} n={n} K={k} T={T} C={C_} H={H} auto_reset={auto_reset}: held pairs {held}, "
          f"envs the twin re-armed {finished}")
    assert_same(snapshot(m, a, EVERYTHING), snapshot(m, b, EVERYTHING), "mppi(commit) vs the chosen tape")
    for key in ("reward", "done", "returns"):
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert held >= 2 and a.bad_action_count() == held == b.bad_action_count()
    assert a.version == b.version
    if auto_reset:
        assert int((a.finished() > 0).sum()) > rearmed, "the re-arm path was not exercised"
    a.close()
    b.close()


# ---- 7. shard invariance ------------------------------------------------------------------------------------------------
def test_two_shards_equal_one_handle(m):
    n, k, T, C_, H, tol = 2048, 7, 6, 5, 2, 20.0
    mean, sigma = shaped_moments(T, n, 4)
    kw = dict(candidates=C_, temperature=1.5, draw=1, seed=PLAN_SEED, commit=H, auto_reset=True, fit_sigma=True, all_returns=True,
              weights=True, returns=True)
    whole = make_engine(m, "ref", n, k, tol)
    whole.reset_random(SEED, 0)
    want = host(whole.mppi(dev(whole, mean), dev(whole, sigma), **kw))
    state = snapshot(m, whole, ("F_GOALS", "F_POINTS", "F_ALIVE", "F_TOTAL_REWARD", "F_EPISODES"))
    for base in (0, 1024):
        part = make_engine(m, "ref", 1024, k, tol, env_id_base=base)
        part.reset_random(SEED, 0)
        sl = slice(base, base + 1024)
        got = host(part.mppi(dev(part, mean[:, :, sl]), dev(part, sigma[:, :, sl]), **kw))
        for key in want:
            np.testing.assert_array_equal(got[key], want[key][..., sl], err_msg=f"shard {base} {key}")
        for f, v in snapshot(m, part, tuple(state)).items():
            np.testing.assert_array_equal(v, state[f][sl], err_msg=f"shard {base} {f}")
        part.close()
    assert len(np.unique(want["best"])) == C_
    whole.close()


# ---- 8. against the fp64 oracle -----------------------------------------------------------------------------------------
def test_every_drawn_candidate_against_the_c_oracle(m):
    """tests/test_gpu_cem.py's inputs for the same check: the block is the same one, so its clean share is (>= 0.90)."""
    from oracle import c_oracle
    table_name, n, k, T, C_, tol = "ref", 3001, 7, 8, 6, 20.0
    table, radius = _table(m, table_name)
    mean, sigma = shaped_moments(T, n, 4)
    eng = started(m, table_name, n, k, tol, history(C_, T, n, 4))
    kw = dict(candidates=C_, draw=6, seed=PLAN_SEED)
    mean_d, sigma_d = dev(eng, mean), dev(eng, sigma)
    plans = eng.sample_plans(mean_d, sigma_d, **kw).cpu().numpy().transpose(0, 1, 3, 2)     # (C, T, n, D)
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
    res = host(eng.mppi(mean_d, sigma_d, temperature=1.5, all_returns=True, **kw))
    print(f"[mppi-vs-oracle] {table_name} n={n} K={k} T={T} C={C_} tol={tol}: clean share {clean.mean():.4f}")
    assert clean.mean() >= 0.90, clean.mean()
    np.testing.assert_array_equal(res["candidate_returns"][:, clean], want[:, clean].astype(np.float32))
    np.testing.assert_array_equal(res["best"][clean], np.argmax(want, axis=0)[clean])
    np.testing.assert_array_equal(res["best_return"][clean], want.max(axis=0)[clean].astype(np.float32))
    eng.close()


# ---- 9. errors, stream order, capture -----------------------------------------------------------------------------------
def test_error_returns_and_dispatch_entry(m):
    import torch
    L = m.lib
    n, T, D, C_ = 3001, 3, 4, 4
    eng = make_engine(m, "ref", n, 7, 8.0)
    device = torch.device("cuda", eng.device)
    rows = torch.zeros((4 * T * D + 1, n), dtype=torch.float32, device=device)
    mean, sigma, mean_out, sigma_out = (rows[q * T * D:(q + 1) * T * D] for q in range(4))
    chosen = torch.zeros((T * D, n), dtype=torch.float32, device=device)
    logs = torch.zeros((max(T, C_), n), dtype=torch.float32, device=device)
    long_rows = torch.zeros((128 * D, n), dtype=torch.float32, device=device)
    torch.cuda.synchronize(device)

    def call(engine=eng, **over):
        arg = L.MtMppi()
        arg.struct_size, arg.n_steps, arg.n_candidates, arg.decay = C.sizeof(L.MtMppi), T, C_, 0.5
        arg.mean, arg.sigma, arg.ld = mean.data_ptr(), sigma.data_ptr(), n
        arg.lo, arg.hi, arg.chosen_ld, arg.out_ld = -180.0, 180.0, n, n
        for key, v in over.items():
            setattr(arg, key, v)
        rc = engine._lib.mt_mppi(engine._h, C.byref(arg))
        return rc, engine._lib.mt_last_error(engine._h).decode()

    rc, msg = call()
    assert rc == L.MT_ERR_STATE and "reset" in msg                              # before a reset
    eng.reset_random(SEED, 0)
    assert call()[0] == L.MT_OK                                                 # no output at all
    assert call(mean_out=mean_out.data_ptr())[0] == L.MT_OK                     # the mean alone
    assert call(mean_out=mean_out.data_ptr(), sigma_out=sigma_out.data_ptr())[0] == L.MT_OK
    assert call(mean_out=mean.data_ptr())[0] == L.MT_OK                         # exactly in place, the mean alone
    assert call(mean_out=mean.data_ptr(), sigma_out=sigma.data_ptr())[0] == L.MT_OK
    assert call(decay=0.0)[0] == L.MT_OK and call(decay=1.0)[0] == L.MT_OK
    assert call(n_steps=127, mean=long_rows.data_ptr(), sigma=long_rows.data_ptr())[0] == L.MT_OK      # the longest horizon
    assert call(commit_steps=T, chosen_out=chosen.data_ptr(), log_ld=0)[0] == L.MT_OK         # no log given: the pitch is not looked at
    eng.reset_random(SEED, 0)
    eng.sync()
    rows.zero_()
    chosen.zero_()
    torch.cuda.synchronize(device)
    before = snapshot(m, eng, EVERYTHING)
    nan, inf = float("nan"), float("inf")
    for over, field in ((dict(struct_size=C.sizeof(L.MtMppi) - 8), "struct_size"),
                        (dict(reserved=1), "reserved"),
                        (dict(flags=0x4), "flags"),
                        (dict(n_steps=-1), "n_steps"),
                        (dict(n_steps=128, mean=long_rows.data_ptr(), sigma=long_rows.data_ptr()), "n_steps"),       # T > 127
                        (dict(n_candidates=0), "n_candidates"),
                        (dict(n_candidates=65), "n_candidates"),                             # C > 64
                        (dict(commit_steps=-1), "commit_steps"),
                        (dict(commit_steps=T + 1, chosen_out=chosen.data_ptr()), "commit_steps"),      # H > T
                        (dict(flags=L.MPPI_AUTO_RESET), "commit_steps"),                     # AUTO_RESET with H = 0
                        (dict(commit_steps=1), "chosen_out"),                                # H > 0 without chosen_out
                        (dict(commit_steps=1, chosen_out=chosen.data_ptr(), chosen_ld=n - 1), "chosen_ld"),
                        (dict(commit_steps=1, chosen_out=mean.data_ptr()), "chosen_out overlaps"),
                        (dict(commit_steps=1, chosen_out=mean_out.data_ptr(), mean_out=mean_out.data_ptr()), "chosen_out overlaps"),
                        (dict(decay=-0.1), "decay"), (dict(decay=1.5), "decay"), (dict(decay=nan), "decay"), (dict(decay=inf), "decay"),
                        (dict(lo=nan), "lo"), (dict(hi=nan), "hi"), (dict(lo=-inf), "lo"), (dict(hi=40000.0), "hi"),
                        (dict(lo=10.0, hi=-10.0), "lo"),
                        (dict(sigma_min=nan), "sigma_min"), (dict(sigma_min=inf), "sigma_min"), (dict(sigma_min=-1.0), "sigma_min"),
                        (dict(mean=None), "mean"), (dict(sigma=None), "sigma"),
                        (dict(ld=n - 1), "ld"),
                        (dict(sigma_out=sigma_out.data_ptr()), "sigma_out without mean_out"),
                        (dict(mean_out=mean_out.data_ptr(), out_ld=n - 1), "out_ld"),
                        (dict(mean_out=mean.data_ptr() + 4 * n), "mean_out overlaps mean"),   # one row down
                        (dict(mean_out=mean.data_ptr(), ld=n, out_ld=n + 1), "mean_out overlaps mean"),
                        (dict(mean_out=mean_out.data_ptr(), sigma_out=sigma.data_ptr() + 4 * n), "sigma_out overlaps sigma"),
                        (dict(mean_out=sigma.data_ptr()), "mean_out overlaps sigma"),
                        (dict(mean_out=sigma.data_ptr(), sigma_out=mean.data_ptr()), "overlaps"),      # swapped
                        (dict(mean_out=mean_out.data_ptr(), sigma_out=mean_out.data_ptr() + 8), "mean_out overlaps sigma_out"),
                        (dict(returns_out=logs.data_ptr(), ret_ld=n - 1), "ret_ld"),
                        (dict(weights_out=logs.data_ptr(), w_ld=n - 1), "w_ld"),
                        (dict(commit_steps=1, chosen_out=chosen.data_ptr(), reward_log=logs.data_ptr(), log_ld=n - 1), "log_ld")):
        rc, msg = call(**over)
        assert rc == L.MT_ERR_INVALID_ARG and field in msg, (over, rc, msg)
    assert call(n_steps=0, mean=None, sigma=None)[0] == L.MT_OK                 # T = 0: a no-op
    eng.sync()
    assert_same(snapshot(m, eng, EVERYTHING), before, "after the refused calls and T = 0")
    assert not rows.any() and not chosen.any() and not logs.any()              # a refusal writes nothing
    version = eng.version
    res = eng.mppi(mean[:0].view(0, D, n), sigma[:0].view(0, D, n), candidates=C_, decay=0.5)
    assert res["best"].shape == (n,) and res["weight_sum"].shape == (n,) and eng.version == version
    with pytest.raises(ValueError):
        eng.mppi(mean.view(T, D, n), sigma.view(T, D, n), candidates=C_, decay=0.5, commit=T + 1)
    with pytest.raises(ValueError):
        eng.mppi(mean.view(T, D, n)[:, :, ::2], sigma.view(T, D, n), candidates=C_, decay=0.5)

    tr = make_engine(m, "ref", n, 7, 8.0, trace=True)
    tr.reset_random(SEED, 0)
    rc, msg = call(engine=tr)
    assert rc == L.MT_ERR_UNSUPPORTED and "mt_mppi: not available on a handle with MT_FLAG_TRACE" in msg
    with pytest.raises(m.ManytorError):
        tr.mppi(mean.view(T, D, n), sigma.view(T, D, n), candidates=C_, decay=0.5)
    assert tr.dispatch()["mppi"]["usable"] is False
    assert eng.dispatch()["mppi"] == {"usable": True, "envs_per_block": 64, "waves_per_block": 4, "max_candidates": 64,
                                      "max_steps": 127}
    assert eng.dispatch()["cem"] == {"usable": True, "envs_per_block": 64, "waves_per_block": 4, "max_candidates": 64}
    tr.close()
    eng.close()


def test_mppi_is_ordered_with_torch_ops_on_the_callers_stream(m):
    import torch
    n, k, T, C_, H, tol = 3001, 7, 8, 6, 3, 20.0
    mean, sigma = shaped_moments(T, n, 4)
    hist = history(C_, T, n, 4)
    kw = dict(candidates=C_, temperature=1.5, seed=PLAN_SEED, commit=H, auto_reset=True, fit_sigma=True, returns=True)
    own = started(m, "ref", n, k, tol, hist)
    want = host(own.mppi(dev(own, mean), dev(own, sigma), **kw))
    own.sync()

    eng = make_engine(m, "ref", n, k, tol)
    eng.use_torch_stream()
    eng.reset_random(SEED, 0)
    eng.rollout_actions(hist)
    device = torch.device("cuda", eng.device)
    src, sigma_d = dev(eng, mean), dev(eng, sigma)
    buf = torch.zeros_like(src)
    ballast = torch.ones((2048, 2048), device=device)
    torch.cuda.synchronize(device)
    for _ in range(8):                                             # keeps the stream busy ahead of the mean's writer
        ballast = ballast @ ballast * 1e-4
    buf.copy_(src)                                                 # the torch op that writes the mean ...
    res = eng.mppi(buf, sigma_d, inplace=True, **kw)               # ... read and refitted in place, no host sync ...
    shifted = torch.roll(res["mean"], -H, dims=0)                  # ... and a torch op on the refit right behind
    hist_best = torch.bincount(res["best"].to(torch.int64), minlength=C_)
    torch.cuda.synchronize(device)
    np.testing.assert_array_equal(hist_best.cpu().numpy(), np.bincount(want["best"], minlength=C_))
    np.testing.assert_array_equal(shifted.cpu().numpy(), np.roll(want["mean"], -H, axis=0))
    for key in ("best", "best_return", "weight_sum", "returns", "chosen", "sigma"):
        np.testing.assert_array_equal(res[key].cpu().numpy(), want[key], err_msg=key)
    assert_same(snapshot(m, eng, EVERYTHING), snapshot(m, own, EVERYTHING), "caller's stream vs own stream")
    eng.close()
    own.close()


def test_mppi_is_capturable_in_a_hip_graph(m):
    """One linear capture on one side stream records `static_mean.copy_(staging); mt_mppi(in place, commit = H)` with
    preallocated outputs; one replay equals the eager call on a twin: outputs and the state behind them."""
    import torch
    L = m.lib
    n, k, T, C_, H, D, tol = 3001, 7, 6, 5, 2, 4, 20.0
    mean, sigma = shaped_moments(T, n, D)
    eager, graphed = make_engine(m, "ref", n, k, tol), make_engine(m, "ref", n, k, tol)
    for e in (eager, graphed):
        e.use_torch_stream()
        e.reset_random(SEED, 0)
    device = torch.device("cuda", graphed.device)
    staging = torch.zeros((T, D, n), dtype=torch.float32, device=device)       # refreshed in front of the replay
    static_mean, static_sigma = torch.zeros_like(staging), dev(graphed, sigma)
    best = torch.zeros((n,), dtype=torch.int32, device=device)
    best_ret = torch.zeros((n,), dtype=torch.float32, device=device)
    wsum = torch.zeros((n,), dtype=torch.float32, device=device)
    wts = torch.zeros((C_, n), dtype=torch.float32, device=device)
    chosen = torch.zeros((H, D, n), dtype=torch.float32, device=device)
    rew = torch.zeros((H, n), dtype=torch.int8, device=device)
    done = torch.zeros((H, n), dtype=torch.uint8, device=device)
    ret = torch.zeros((n,), dtype=torch.float32, device=device)
    decay = float(mppi_ref.decay_of(1.5))
    arg = L.MtMppi()
    arg.struct_size, arg.n_steps, arg.n_candidates, arg.commit_steps = C.sizeof(L.MtMppi), T, C_, H
    arg.draw, arg.decay, arg.lo, arg.hi, arg.sigma_min = 4, decay, -180.0, 180.0, 0.0
    arg.mean, arg.sigma, arg.ld = static_mean.data_ptr(), static_sigma.data_ptr(), n
    arg.mean_out, arg.sigma_out, arg.out_ld = static_mean.data_ptr(), static_sigma.data_ptr(), n
    arg.best_out, arg.best_return_out, arg.weight_sum_out = best.data_ptr(), best_ret.data_ptr(), wsum.data_ptr()
    arg.weights_out, arg.w_ld = wts.data_ptr(), n
    arg.chosen_out, arg.chosen_ld = chosen.data_ptr(), n
    arg.reward_log, arg.done_log, arg.log_ld, arg.return_out = rew.data_ptr(), done.data_ptr(), n, ret.data_ptr()
    arg.seed, arg.flags = PLAN_SEED, L.MPPI_AUTO_RESET
    side = torch.cuda.Stream(device=device)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(side):
        graphed.use_torch_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static_mean.copy_(staging)
            rc = graphed._lib.mt_mppi(graphed._h, C.byref(arg))
    assert rc == L.MT_OK, graphed._lib.mt_last_error(graphed._h)
    torch.cuda.synchronize(device)
    graphed.reset_random(SEED, 0)         # the capture pass itself does not execute; start from the same state anyway
    torch.cuda.synchronize(device)
    want = host(eager.mppi(dev(eager, mean), dev(eager, sigma), candidates=C_, decay=decay, draw=4, seed=PLAN_SEED, commit=H,
                           auto_reset=True, fit_sigma=True, weights=True, log=True, returns=True))
    staging.copy_(dev(graphed, mean))
    graph.replay()
    torch.cuda.synchronize(device)
    for key, got in (("best", best), ("best_return", best_ret), ("weight_sum", wsum), ("weights", wts), ("chosen", chosen),
                     ("reward", rew), ("done", done), ("returns", ret), ("mean", static_mean), ("sigma", static_sigma)):
        np.testing.assert_array_equal(got.cpu().numpy(), want[key], err_msg=key)
    assert np.abs(want["reward"]).sum() > 0
    assert_same(snapshot(m, graphed, EVERYTHING), snapshot(m, eager, EVERYTHING), "replay")
    eager.close()
    graphed.close()
