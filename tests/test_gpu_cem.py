"""mt_cem / StepEngine.cem and mt_sample_plans / StepEngine.sample_plans: one iteration of the cross-entropy method in one
call, the candidates drawn in the kernel.

Held to:
  * tests/cem_ref.py, the numpy restatement of the candidate stream, the elite rule and the refit (bit for bit; the
    hardware square root of sigma_out within 1 ulp);
  * the calls that already exist: the evaluation == shoot() on the block sample_plans() writes, a commit == rollout_actions(
    chosen) on a twin handle, every field;
  * the fp64 C restatement of the reference (oracle/manytor_oracle.c) for every candidate of every env whose decision
    margins stay outside GUARD (tests/test_gpu_shoot.py: same rule).

Inputs unless a test says otherwise: reset_random(SEED, 0) and test_gpu_shoot's two history steps; a mean drawn uniformly in
+-150 degrees with joints 1 and 2 scaled by 0.4, a sigma drawn in 5..60 degrees, lo / hi = -+180: the clamp bites.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cem_ref
from parity_util import GUARD
from test_gpu_shoot import SHAPE, dry_runs, host, shaped_plans, started
from test_gpu_tape import EVERYTHING, SEED, _table, assert_same, make_engine, snapshot, unusable

pytestmark = pytest.mark.gpu

PLAN_SEED = 0xC0FFEE12345


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


@functools.lru_cache(maxsize=None)
def shaped_moments(T, n, D):
    """(mean, sigma), (T, D, n) float32, read-only."""
    rng = np.random.RandomState(SEED + 7 * T + n)
    mean = rng.uniform(-150, 150, (T, D, n)).astype(np.float32)
    mean[:, 1:3] *= SHAPE
    sigma = rng.uniform(5, 60, (T, D, n)).astype(np.float32)
    mean.setflags(write=False)
    sigma.setflags(write=False)
    return mean, sigma


@functools.lru_cache(maxsize=None)
def turns_moments(T, n, D):
    """test_gpu_tape.turns_tape's recipe for the mean: small angles plus whole turns out to +-32 400 degrees."""
    rng = np.random.RandomState(SEED + 7 * T + n)
    mean = (rng.uniform(-60, 60, (T, D, n)) + 360.0 * rng.randint(-90, 91, (1, D, n))).astype(np.float32)
    sigma = rng.uniform(1, 20, (T, D, n)).astype(np.float32)
    mean.setflags(write=False)
    sigma.setflags(write=False)
    return mean, sigma


def dev(eng, a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(torch.device("cuda", eng.device))      # (a copy: the inputs are read-only)


def ids(eng):
    return np.uint64(eng.env_id_base) + np.arange(eng.n_envs, dtype=np.uint64)


def history(C_, T, n, D):
    return shaped_plans(C_, T, n, D)[1]


# table, n, K, T, C, tol, kind, env_id_base, draw, keep_mean
CASES = [
    ("ref", 3001, 7, 8, 6, 20.0, "shaped", 0, 0, False),           # n % 64 != 0, C % 4 != 0
    ("dh7", 5003, 3, 6, 5, 45.0, "shaped", 0, 3, True),            # 7 joints: block 1 in use; candidate 0 is the mean
    ("rt5", 1501, 3, 5, 3, 8.0, "shaped", 0, 1, False),            # 5 joints: one word of block 1; a wave without candidates
    ("ref", 777, 7, 3, 64, 20.0, "shaped", 0, 2, True),            # C = 64: c << 24 uses its whole field
    ("ref", 3001, 7, 8, 6, 20.0, "shaped", (1 << 33) + 12345, 7, False),      # env ids with a high word
    ("ref", 3001, 7, 6, 5, 8.0, "turns", 0, 4, False),             # |angle| > 30 000: the wide form, lo / hi = -+32768
]


def case_inputs(m, case):
    table_name, n, k, T, C_, tol, kind, base, draw, keep = case
    D = len(_table(m, table_name)[0])
    mean, sigma = (shaped_moments if kind == "shaped" else turns_moments)(T, n, D)
    lim = 180.0 if kind == "shaped" else 32768.0
    eng = started(m, table_name, n, k, tol, history(C_, T, n, D), env_id_base=base)
    kw = dict(candidates=C_, draw=draw, seed=PLAN_SEED, lo=-lim, hi=lim, keep_mean=keep)
    return eng, mean, sigma, kw


# ---- 1. the candidate stream == the restatement -----------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-C{c[4]}-{c[6]}-base{c[7]}")
def test_sample_plans_equals_the_restatement_bit_for_bit(m, case):
    eng, mean, sigma, kw = case_inputs(m, case)
    C_, kind, keep = case[4], case[6], case[9]
    got = eng.sample_plans(dev(eng, mean), dev(eng, sigma), **kw).cpu().numpy()
    want = cem_ref.sample_plans(PLAN_SEED, ids(eng), kw["draw"], C_, mean, sigma, kw["lo"], kw["hi"], keep)
    assert got.shape == want.shape and got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    clamped = (np.abs(got) == np.float32(kw["hi"])).mean()
    print(f"[cem-stream] {case}: clamped share {clamped:.4f}, distinct values {len(np.unique(got))}")
    if kind == "shaped":
        assert clamped > 0.001, clamped                            # the clamp really bites on these inputs
    if keep:
        np.testing.assert_array_equal(got[0], np.clip(mean, np.float32(kw["lo"]), np.float32(kw["hi"])))
    else:
        assert (got[0] != mean).mean() > 0.9
    other = eng.sample_plans(dev(eng, mean), dev(eng, sigma), **dict(kw, draw=kw["draw"] + 1)).cpu().numpy()
    assert (other[-1] != got[-1]).mean() > 0.9                     # another draw: another block
    eng.close()


# ---- 2. evaluation == shoot() on the sampled block ----------------------------------------------------------------------
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
    got = host(eng.cem(mean_d, sigma_d, elites=max(1, C_ // 2), all_returns=True, **kw))
    differ = (want["candidate_returns"].max(axis=0) != want["candidate_returns"].min(axis=0)).mean()
    print(f"[cem-vs-shoot] {case}: envs whose candidates differ {differ:.3f}, mean best return {want['best_return'].mean():+.3f}")
    assert got["candidate_returns"].dtype == np.float32 and got["best"].dtype == np.int32
    np.testing.assert_array_equal(got["candidate_returns"], want["candidate_returns"])
    np.testing.assert_array_equal(got["best"], want["best"])
    np.testing.assert_array_equal(got["best_return"], want["best_return"])
    assert differ > 0.05, differ
    eng.close()


# ---- 3. elites and refit ------------------------------------------------------------------------------------------------
def ulps(a, b):
    a, b = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(a - b)


# `straddle`: half of the share of envs whose E-th and (E+1)-th best returns are equal (a tie across the elite boundary) on
# these inputs, by the dry runs: 0.3312, -, 0.9472, 0.6934.  The floor shows that the tie rule is at work.
@pytest.mark.parametrize("table_name,n,k,T,C_,E,tol,sigma_min,straddle", [
    ("ref", 3001, 7, 8, 6, 1, 20.0, 0.5, 0.165),
    ("ref", 3001, 7, 8, 6, 6, 20.0, 0.0, 0.0),                     # E = C: no boundary inside the set
    ("ref", 777, 7, 3, 64, 16, 20.0, 2.0, 0.47),                   # E = C / 4 at C = 64
    ("dh7", 5003, 3, 6, 5, 2, 45.0, 8.0, 0.34),
])
def test_elites_and_refit_equal_the_restatement(m, table_name, n, k, T, C_, E, tol, sigma_min, straddle):
    """elite_mask against the restated rule on the returned scores (which equal the dry runs), mean_out bit for bit,
    sigma_out within 1 ulp (a hardware square root may be 1 ulp off; measured: 0) and exactly sigma_min under the floor."""
    D = len(_table(m, table_name)[0])
    mean, sigma = shaped_moments(T, n, D)
    eng = started(m, table_name, n, k, tol, history(C_, T, n, D))
    kw = dict(candidates=C_, draw=9, seed=PLAN_SEED)
    mean_d, sigma_d = dev(eng, mean), dev(eng, sigma)
    block = eng.sample_plans(mean_d, sigma_d, **kw).cpu().numpy()
    got = host(eng.cem(mean_d, sigma_d, elites=E, sigma_min=sigma_min, all_returns=True, elite_mask=True, **kw))
    scores = got["candidate_returns"]
    np.testing.assert_array_equal(scores, dry_runs(eng, block.transpose(0, 1, 3, 2)))
    ranked = -np.sort(-scores, axis=0)
    share = float((ranked[E - 1] == ranked[E]).mean()) if E < C_ else 0.0
    print(f"[cem-elites] {table_name} n={n} C={C_} E={E}: envs with a tie straddling the elite boundary {share:.4f}")
    assert share >= straddle, (share, straddle)
    mask = got["elite_mask"].view(np.uint64)
    np.testing.assert_array_equal(mask, cem_ref.elite_mask(scores, E))
    assert (np.array([bin(int(v)).count("1") for v in mask]) == E).all()
    assert ((mask >> got["best"].astype(np.uint64)) & np.uint64(1)).all()      # the best is an elite
    want_m, want_s = cem_ref.refit(block, scores, E, sigma_min)
    np.testing.assert_array_equal(got["mean"], want_m)
    worst = int(ulps(got["sigma"], want_s).max())
    floored = want_s == np.float32(sigma_min)
    print(f"[cem-refit] sigma_out: worst distance {worst} ulp, floored share {floored.mean():.4f}")
    assert worst <= 1, worst
    assert (got["sigma"] >= np.float32(sigma_min)).all()
    raw_s = cem_ref.refit(block, scores, E, 0.0)[1]
    clearly = raw_s * np.float32(1.000001) < np.float32(sigma_min)             # below the floor by more than an ulp
    np.testing.assert_array_equal(got["sigma"][clearly], np.float32(sigma_min))
    if E == 1:
        assert floored.all() and clearly.all() == (sigma_min > 0)
    eng.close()


def test_sigma_zero_makes_every_candidate_the_mean(m):
    n, k, T, C_, E, tol = 3001, 7, 8, 6, 3, 20.0
    mean, _ = shaped_moments(T, n, 4)
    eng = started(m, "ref", n, k, tol, history(C_, T, n, 4))
    mean_d = dev(eng, mean)
    got = host(eng.cem(mean_d, mean_d * 0, candidates=C_, elites=E, sigma_min=1.25, seed=PLAN_SEED, all_returns=True,
                       elite_mask=True))
    scores = got["candidate_returns"]
    np.testing.assert_array_equal(scores, np.broadcast_to(scores[0], scores.shape))
    np.testing.assert_array_equal(scores[0], dry_runs(eng, mean.transpose(0, 2, 1)[None])[0])
    assert (got["best"] == 0).all() and (got["elite_mask"] == (1 << E) - 1).all()
    np.testing.assert_array_equal(got["sigma"], np.float32(1.25))
    np.testing.assert_allclose(got["mean"], mean, rtol=3e-7, atol=0)           # (x + x + x) * fl(1 / 3): two roundings
    eng.close()


# ---- 4. in place == out of place ----------------------------------------------------------------------------------------
def test_in_place_refit_equals_out_of_place(m):
    n, k, T, C_, E, H, tol = 3001, 7, 8, 6, 2, 2, 20.0
    mean, sigma = shaped_moments(T, n, 4)
    a = started(m, "ref", n, k, tol, history(C_, T, n, 4))
    b = started(m, "ref", n, k, tol, history(C_, T, n, 4))
    kw = dict(candidates=C_, elites=E, seed=PLAN_SEED, draw=2, commit=H, sigma_min=0.5, all_returns=True, elite_mask=True,
              keep_mean=True)
    mean_a, sigma_a, mean_b, sigma_b = dev(a, mean), dev(a, sigma), dev(b, mean), dev(b, sigma)
    out = a.cem(mean_a, sigma_a, **kw)
    inp = b.cem(mean_b, sigma_b, inplace=True, **kw)
    assert inp["mean"] is mean_b and inp["sigma"] is sigma_b and out["mean"] is not mean_a
    np.testing.assert_array_equal(mean_a.cpu().numpy(), mean)                  # out of place: the inputs stay
    out, inp = host(out), host(inp)
    assert (out["mean"] != mean).mean() > 0.9
    for key in out:
        np.testing.assert_array_equal(inp[key], out[key], err_msg=key)
    assert_same(snapshot(m, b, EVERYTHING), snapshot(m, a, EVERYTHING), "in place vs out of place")
    a.close()
    b.close()


# ---- 5. an evaluation changes nothing resident; a NaN stays in its env -------------------------------------------------
def test_evaluate_only_changes_nothing_resident_and_a_nan_stays_in_its_env(m):
    n, k, T, C_, E, tol, env = 3001, 7, 8, 6, 2, 20.0, 1000
    mean, sigma = shaped_moments(T, n, 4)
    hist = history(C_, T, n, 4)
    eng = started(m, "ref", n, k, tol, hist)
    eng.set_actions(hist[1] + np.float32(0.5))                     # an action row that no call below would write
    before = snapshot(m, eng, EVERYTHING)
    bad_before, version = eng.bad_action_count(), eng.version
    kw = dict(candidates=C_, elites=E, seed=PLAN_SEED, all_returns=True, elite_mask=True)
    clean = host(eng.cem(dev(eng, mean), dev(eng, sigma), **kw))
    planted = mean.copy()
    planted[:, 2, env] = np.nan                                    # every step of one env: its candidates hold the pose
    got = host(eng.cem(dev(eng, planted), dev(eng, sigma), **kw))
    eng.sync()
    assert_same(snapshot(m, eng, EVERYTHING), before, "after two evaluations")
    assert eng.bad_action_count() == bad_before and eng.version == version
    others = np.arange(n) != env
    for key in clean:
        np.testing.assert_array_equal(got[key][..., others], clean[key][..., others], err_msg=key)
    held = np.full((1, T, n, 4), np.nan, dtype=np.float32)
    np.testing.assert_array_equal(got["candidate_returns"][:, env], np.repeat(dry_runs(eng, held)[0, env], C_))
    assert got["best"][env] == 0 and got["elite_mask"][env] == (1 << E) - 1
    eng.close()


# ---- 6. commit == rollout_actions(chosen) on a twin handle -------------------------------------------------------------
# `rearmed`: half of the number of envs the twin's own rollout_actions(chosen) finishes on these inputs -- 25 (ref, H = 3 of
# T = 8) and 2 997 (dh7, H = T) -- the floor of the re-arm check
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
    got = a.cem(mean_d, sigma_d, elites=2, commit=H, auto_reset=auto_reset, log=True, returns=True, **kw)
    a.sync()
    chosen = got["chosen"]
    got = host(got)
    np.testing.assert_array_equal(got["chosen"].view(np.uint32),
                                  block[got["best"], :H, :, np.arange(n)].transpose(1, 2, 0).view(np.uint32))
    want = host(b.rollout_actions(chosen, layout="soa", auto_reset=auto_reset, seed=PLAN_SEED, log=True, returns=True))
    b.sync()
    held = sum(int(unusable(got["chosen"][t].T).sum()) for t in range(H))
    finished = int((b.finished() > 0).sum())
    print(f"[cem-commit] {table_name} n={n} K={k} T={T} C={C_} H={H} auto_reset={auto_reset}: held pairs {held}, "
          f"envs the twin re-armed {finished}")
    assert_same(snapshot(m, a, EVERYTHING), snapshot(m, b, EVERYTHING), "cem(commit) vs the chosen tape")
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
    n, k, T, C_, E, H, tol = 2048, 7, 6, 5, 2, 2, 20.0
    mean, sigma = shaped_moments(T, n, 4)
    kw = dict(candidates=C_, elites=E, draw=1, seed=PLAN_SEED, commit=H, auto_reset=True, all_returns=True, elite_mask=True,
              returns=True)
    whole = make_engine(m, "ref", n, k, tol)
    whole.reset_random(SEED, 0)
    want = host(whole.cem(dev(whole, mean), dev(whole, sigma), **kw))
    state = snapshot(m, whole, ("F_GOALS", "F_POINTS", "F_ALIVE", "F_TOTAL_REWARD", "F_EPISODES"))
    for base in (0, 1024):
        part = make_engine(m, "ref", 1024, k, tol, env_id_base=base)
        part.reset_random(SEED, 0)
        sl = slice(base, base + 1024)
        got = host(part.cem(dev(part, mean[:, :, sl]), dev(part, sigma[:, :, sl]), **kw))
        for key in want:
            np.testing.assert_array_equal(got[key], want[key][..., sl], err_msg=f"shard {base} {key}")
        for f, v in snapshot(m, part, tuple(state)).items():
            np.testing.assert_array_equal(v, state[f][sl], err_msg=f"shard {base} {f}")
        part.close()
    assert len(np.unique(want["best"])) == C_
    whole.close()


# ---- 8. against the fp64 oracle -----------------------------------------------------------------------------------------
def test_every_drawn_candidate_against_the_c_oracle(m):
    """The inputs keep the clean share at 0.90 or more: checked on the CPU with the restatement and the oracle alone (state
    from philox_ref's reset and the oracle's own history steps) before relying on it here."""
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
    res = host(eng.cem(mean_d, sigma_d, elites=2, all_returns=True, **kw))
    print(f"[cem-vs-oracle] {table_name} n={n} K={k} T={T} C={C_} tol={tol}: clean share {clean.mean():.4f}")
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
    logs = torch.zeros((T, n), dtype=torch.uint8, device=device)
    torch.cuda.synchronize(device)

    def call(engine=eng, **over):
        arg = L.MtCem()
        arg.struct_size, arg.n_steps, arg.n_candidates, arg.n_elites = C.sizeof(L.MtCem), T, C_, 2
        arg.mean, arg.sigma, arg.ld = mean.data_ptr(), sigma.data_ptr(), n
        arg.lo, arg.hi, arg.chosen_ld, arg.out_ld = -180.0, 180.0, n, n
        for key, v in over.items():
            setattr(arg, key, v)
        rc = engine._lib.mt_cem(engine._h, C.byref(arg))
        return rc, engine._lib.mt_last_error(engine._h).decode()

    rc, msg = call()
    assert rc == L.MT_ERR_STATE and "reset" in msg                              # before a reset
    eng.reset_random(SEED, 0)
    assert call()[0] == L.MT_OK
    assert call(mean_out=mean_out.data_ptr(), sigma_out=sigma_out.data_ptr())[0] == L.MT_OK
    assert call(mean_out=mean.data_ptr(), sigma_out=sigma.data_ptr())[0] == L.MT_OK          # exactly in place
    assert call(commit_steps=T, chosen_out=chosen.data_ptr(), log_ld=0)[0] == L.MT_OK         # no log given: the pitch is not looked at
    eng.reset_random(SEED, 0)
    eng.sync()
    before = snapshot(m, eng, EVERYTHING)
    nan, inf = float("nan"), float("inf")
    for over, field in ((dict(struct_size=C.sizeof(L.MtCem) - 8), "struct_size"),
                        (dict(reserved=1), "reserved"),
                        (dict(flags=0x4), "flags"),
                        (dict(n_steps=-1), "n_steps"),
                        (dict(n_steps=65536), "n_steps"),                                    # T > 65 535
                        (dict(n_candidates=0), "n_candidates"),
                        (dict(n_candidates=65), "n_candidates"),                             # C > 64
                        (dict(n_elites=0), "n_elites"),
                        (dict(n_elites=C_ + 1), "n_elites"),                                 # E > C
                        (dict(commit_steps=-1), "commit_steps"),
                        (dict(commit_steps=T + 1, chosen_out=chosen.data_ptr()), "commit_steps"),      # H > T
                        (dict(flags=L.CEM_AUTO_RESET), "commit_steps"),                      # AUTO_RESET with H = 0
                        (dict(commit_steps=1), "chosen_out"),                                # H > 0 without chosen_out
                        (dict(commit_steps=1, chosen_out=chosen.data_ptr(), chosen_ld=n - 1), "chosen_ld"),
                        (dict(commit_steps=1, chosen_out=mean.data_ptr()), "chosen_out overlaps"),
                        (dict(lo=nan), "lo"), (dict(hi=nan), "hi"), (dict(lo=-inf), "lo"), (dict(hi=40000.0), "hi"),
                        (dict(lo=10.0, hi=-10.0), "lo"),
                        (dict(sigma_min=nan), "sigma_min"), (dict(sigma_min=inf), "sigma_min"), (dict(sigma_min=-1.0), "sigma_min"),
                        (dict(mean=None), "mean"), (dict(sigma=None), "sigma"),
                        (dict(ld=n - 1), "ld"),
                        (dict(mean_out=mean_out.data_ptr()), "both or neither"),
                        (dict(mean_out=mean_out.data_ptr(), sigma_out=sigma_out.data_ptr(), out_ld=n - 1), "out_ld"),
                        (dict(mean_out=mean.data_ptr() + 4 * n, sigma_out=sigma_out.data_ptr() + 4 * n), "mean_out overlaps mean"),   # one row down
                        (dict(mean_out=mean.data_ptr(), sigma_out=sigma_out.data_ptr(), ld=n, out_ld=n + 1), "mean_out overlaps mean"),
                        (dict(mean_out=sigma.data_ptr(), sigma_out=mean.data_ptr()), "overlaps"),      # swapped
                        (dict(mean_out=mean_out.data_ptr(), sigma_out=mean_out.data_ptr() + 8), "mean_out overlaps sigma_out"),
                        (dict(returns_out=logs.data_ptr(), ret_ld=n - 1), "ret_ld"),
                        (dict(commit_steps=1, chosen_out=chosen.data_ptr(), reward_log=logs.data_ptr(), log_ld=n - 1), "log_ld")):
        rc, msg = call(**over)
        assert rc == L.MT_ERR_INVALID_ARG and field in msg, (over, rc, msg)
    assert call(n_steps=0, mean=None, sigma=None)[0] == L.MT_OK                 # T = 0: a no-op
    arg = L.MtCem()
    arg.n_steps, arg.n_candidates, arg.mean, arg.sigma, arg.ld, arg.lo, arg.hi = T, C_, mean.data_ptr(), sigma.data_ptr(), n, -1.0, 1.0
    for bad_call, field in ((lambda: eng._lib.mt_sample_plans(eng._h, C.byref(arg), None, n, T * D * n), "plans_out"),
                            (lambda: eng._lib.mt_sample_plans(eng._h, C.byref(arg), chosen.data_ptr(), n - 1, T * D * n), "ld"),
                            (lambda: eng._lib.mt_sample_plans(eng._h, C.byref(arg), chosen.data_ptr(), n, T * D * n - 1), "cand_stride")):
        assert bad_call() == L.MT_ERR_INVALID_ARG and field in eng._lib.mt_last_error(eng._h).decode()
    eng.sync()
    assert_same(snapshot(m, eng, EVERYTHING), before, "after the refused calls and T = 0")
    version = eng.version
    res = eng.cem(mean[:0].view(0, D, n), sigma[:0].view(0, D, n), candidates=C_, elites=1)
    assert res["best"].shape == (n,) and eng.version == version
    with pytest.raises(ValueError):
        eng.cem(mean.view(T, D, n), sigma.view(T, D, n), candidates=C_, elites=1, commit=T + 1)
    with pytest.raises(ValueError):
        eng.cem(mean.view(T, D, n)[:, :, ::2], sigma.view(T, D, n), candidates=C_, elites=1)

    tr = make_engine(m, "ref", n, 7, 8.0, trace=True)
    tr.reset_random(SEED, 0)
    rc, msg = call(engine=tr)
    assert rc == L.MT_ERR_UNSUPPORTED and "mt_cem: not available on a handle with MT_FLAG_TRACE" in msg
    with pytest.raises(m.ManytorError):
        tr.cem(mean.view(T, D, n), sigma.view(T, D, n), candidates=C_, elites=1)
    assert tr.dispatch()["cem"]["usable"] is False
    assert eng.dispatch()["cem"] == {"usable": True, "envs_per_block": 64, "waves_per_block": 4, "max_candidates": 64}
    tr.close()
    eng.close()


def test_cem_is_ordered_with_torch_ops_on_the_callers_stream(m):
    import torch
    n, k, T, C_, E, H, tol = 3001, 7, 8, 6, 2, 3, 20.0
    mean, sigma = shaped_moments(T, n, 4)
    hist = history(C_, T, n, 4)
    kw = dict(candidates=C_, elites=E, seed=PLAN_SEED, commit=H, auto_reset=True, returns=True)
    own = started(m, "ref", n, k, tol, hist)
    want = host(own.cem(dev(own, mean), dev(own, sigma), **kw))
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
    res = eng.cem(buf, sigma_d, inplace=True, **kw)                # ... read and refitted in place, no host sync ...
    shifted = torch.roll(res["mean"], -H, dims=0)                  # ... and a torch op on the refit right behind
    hist_best = torch.bincount(res["best"].to(torch.int64), minlength=C_)
    torch.cuda.synchronize(device)
    np.testing.assert_array_equal(hist_best.cpu().numpy(), np.bincount(want["best"], minlength=C_))
    np.testing.assert_array_equal(shifted.cpu().numpy(), np.roll(want["mean"], -H, axis=0))
    for key in ("best", "best_return", "returns", "chosen", "sigma"):
        np.testing.assert_array_equal(res[key].cpu().numpy(), want[key], err_msg=key)
    assert_same(snapshot(m, eng, EVERYTHING), snapshot(m, own, EVERYTHING), "caller's stream vs own stream")
    eng.close()
    own.close()


def test_cem_is_capturable_in_a_hip_graph(m):
    """One linear capture on one side stream records `static_mean.copy_(staging); mt_cem(in place, commit = H)` with
    preallocated outputs; one replay equals the eager call on a twin: outputs and the state behind them."""
    import torch
    L = m.lib
    n, k, T, C_, E, H, D, tol = 3001, 7, 6, 5, 2, 2, 4, 20.0
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
    mask = torch.zeros((n,), dtype=torch.int64, device=device)
    chosen = torch.zeros((H, D, n), dtype=torch.float32, device=device)
    rew = torch.zeros((H, n), dtype=torch.int8, device=device)
    done = torch.zeros((H, n), dtype=torch.uint8, device=device)
    ret = torch.zeros((n,), dtype=torch.float32, device=device)
    arg = L.MtCem()
    arg.struct_size, arg.n_steps, arg.n_candidates, arg.n_elites, arg.commit_steps = C.sizeof(L.MtCem), T, C_, E, H
    arg.draw, arg.lo, arg.hi, arg.sigma_min = 4, -180.0, 180.0, 0.0
    arg.mean, arg.sigma, arg.ld = static_mean.data_ptr(), static_sigma.data_ptr(), n
    arg.mean_out, arg.sigma_out, arg.out_ld = static_mean.data_ptr(), static_sigma.data_ptr(), n
    arg.best_out, arg.best_return_out, arg.elite_mask_out = best.data_ptr(), best_ret.data_ptr(), mask.data_ptr()
    arg.chosen_out, arg.chosen_ld = chosen.data_ptr(), n
    arg.reward_log, arg.done_log, arg.log_ld, arg.return_out = rew.data_ptr(), done.data_ptr(), n, ret.data_ptr()
    arg.seed, arg.flags = PLAN_SEED, L.CEM_AUTO_RESET
    side = torch.cuda.Stream(device=device)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(side):
        graphed.use_torch_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            static_mean.copy_(staging)
            rc = graphed._lib.mt_cem(graphed._h, C.byref(arg))
    assert rc == L.MT_OK, graphed._lib.mt_last_error(graphed._h)
    torch.cuda.synchronize(device)
    graphed.reset_random(SEED, 0)         # the capture pass itself does not execute; start from the same state anyway
    torch.cuda.synchronize(device)
    want = host(eager.cem(dev(eager, mean), dev(eager, sigma), candidates=C_, elites=E, draw=4, seed=PLAN_SEED, commit=H,
                          auto_reset=True, elite_mask=True, log=True, returns=True))
    staging.copy_(dev(graphed, mean))
    graph.replay()
    torch.cuda.synchronize(device)
    for key, got in (("best", best), ("best_return", best_ret), ("elite_mask", mask), ("chosen", chosen), ("reward", rew),
                     ("done", done), ("returns", ret), ("mean", static_mean), ("sigma", static_sigma)):
        np.testing.assert_array_equal(got.cpu().numpy(), want[key], err_msg=key)
    assert np.abs(want["reward"]).sum() > 0
    assert_same(snapshot(m, graphed, EVERYTHING), snapshot(m, eager, EVERYTHING), "replay")
    eager.close()
    graphed.close()
