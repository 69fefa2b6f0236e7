"""mt_es_sample / mt_rollout_population / mt_es (StepEngine.sample_population, .rollout_population, .es,
Multienv.evolve_policy): an evolution-strategies generation on the device.

Held to:
  * tests/es_ref.py, the numpy restatement of the header's definitions, bit for bit and without a tolerance: the
    population, fitness, best, the pair coefficients, grad and the in-place theta (every sum in them is an integer sum);
  * rollout_policy with a member's row as its weights, bit for bit, for everything rollout_population returns, and
    rollout_actions on the logged actions for everything a committing call leaves (the environment semantics are DEFINED by
    those calls; tests/test_gpu_policy.py holds them to the oracle).
Shapes: the smallest that reach each branch -- M = 2 with one block per member, M = 6 with two blocks per member, M = 4 on
the 7-joint table; K = 7, T = 6; one, two and three layers.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import es_ref
import policy_ref
from oracle import philox_ref as px

pytestmark = pytest.mark.gpu

SEED = 0xE5E5
RING = 8
K = 7
T = 6
SIGMA = 0.01

#          table  M  G    widths    hidden  out         see_pose
CONFIGS = {
    "min": ("ref", 2, 256, (), "tanh", "tanh", False),                  # the minimum: one block per member, one layer
    "six": ("ref", 6, 512, (32, 64), "relu", "identity", True),         # two blocks per member, M no power of two, both extents
    "dh7": ("dh7", 4, 256, (5,), "tanh", "tanh", False),                # D > 4, the other table family, a width inside a block of eight
}
ALL = sorted(CONFIGS)

STATE = ("F_GOALS", "F_POINTS", "F_ALIVE", "F_TOTAL_REWARD", "F_EPISODES", "F_LAST_RETURN", "F_RETURN_RING")
OUTPUTS = ("F_OBS", "F_REWARD", "F_DONE", "F_DONE_BITS", "F_EE", "F_ZMIN")
EVERYTHING = ("F_ACTIONS",) + STATE + OUTPUTS
LOGS = dict(log=True, returns=True, actions=True, observations=True)


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def _table(m, name):
    if name == "ref":
        return np.asarray(m.REF_DH_TABLE, dtype=np.float64), 51.3
    return np.asarray(m.DH7_TABLE, dtype=np.float64), 92.6


def make_engine(m, cfg, n=None, tol=8.0, **kw):
    name, M, G = CONFIGS[cfg][:3]
    table, radius = _table(m, name)
    return m.StepEngine(M * G if n is None else n, K, dh_table=table, radius=radius, pickup_tol=tol, return_ring=RING, debug_zmin=True,
                        **kw)


def dof_of(cfg):
    return 4 if CONFIGS[cfg][0] == "ref" else 7


def n_inputs(cfg):
    return 3 * K + (dof_of(cfg) if CONFIGS[cfg][6] else 0)


@functools.lru_cache(maxsize=None)
def host_theta(cfg):
    layers = policy_ref.make_weights(SEED + len(cfg), n_inputs(cfg), CONFIGS[cfg][3], dof_of(cfg))
    theta = np.concatenate([t.reshape(-1) for pair in layers for t in pair]).astype(np.float32)
    theta.setflags(write=False)
    return theta


@functools.lru_cache(maxsize=None)
def host_population(cfg, draw=0):
    pop = es_ref.sample_population(host_theta(cfg), SIGMA, CONFIGS[cfg][1], draw, SEED)
    pop.setflags(write=False)
    return pop


def policy_kw(cfg, **over):
    _, _, _, widths, hidden, out, see_pose = CONFIGS[cfg]
    kw = dict(widths=widths, hidden=hidden, out=out, see_pose=see_pose, seed=SEED)
    kw.update(over)
    return kw


def layer_kw(cfg, **over):
    kw = policy_kw(cfg, **over)
    del kw["widths"]
    return kw


def to_dev(eng, a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", eng.device))


def to_np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def snapshot(m, eng, fields=EVERYTHING):
    return {f: eng.get(getattr(m.lib, f)) for f in fields}


def assert_same(got, want, what=""):
    assert got.keys() == want.keys()
    for f in want:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what} {f}")


# ---- 1. the population ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ALL)
def test_sample_population_is_the_restatement(m, cfg):
    import torch
    eng = make_engine(m, cfg)
    M = CONFIGS[cfg][1]
    theta = to_dev(eng, host_theta(cfg))
    assert theta.numel() == eng.policy_size(CONFIGS[cfg][3], CONFIGS[cfg][6])
    got = {d: eng.sample_population(theta, SIGMA, members=M, draw=d, seed=SEED).cpu().numpy() for d in (0, 3)}
    for d in (0, 3):
        np.testing.assert_array_equal(got[d], es_ref.sample_population(host_theta(cfg), SIGMA, M, d, SEED), err_msg=f"draw {d}")
    assert np.mean(got[0] != got[3]) > 0.9
    np.testing.assert_array_equal(theta.cpu().numpy(), host_theta(cfg))
    if cfg == "dh7":                                                     # pitch > P: the words past P stay the caller's
        P = theta.numel()
        out = torch.full((M, P + 5), 7.0, dtype=torch.float32, device=theta.device)
        assert eng.sample_population(theta, SIGMA, members=M, draw=3, seed=SEED, out=out) is out
        np.testing.assert_array_equal(out[:, :P].cpu().numpy(), got[3])
        assert bool((out[:, P:] == 7.0).all())
        view = torch.full((M, 2 * P + 3), -1.0, dtype=torch.float32, device=theta.device)[:, 1:P + 1]      # rows not at the pitch's start
        eng.sample_population(theta, SIGMA, members=M, draw=0, seed=SEED, out=view)
        np.testing.assert_array_equal(view.cpu().numpy(), got[0])
    eng.close()


# ---- 2. scoring is rollout_policy with the member's row ---------------------------------------------------------------
@pytest.mark.parametrize("cfg", ALL)
def test_every_member_gets_what_rollout_policy_gives_its_row(m, cfg):
    _, M, G, widths, _, _, see_pose = CONFIGS[cfg]
    eng = make_engine(m, cfg)
    eng.reset_random(SEED, 0)
    pop = to_dev(eng, host_population(cfg))
    before = snapshot(m, eng)
    res = to_np(eng.rollout_population(pop, T, **policy_kw(cfg, dry_run=True, **LOGS)))
    eng.sync()
    assert_same(snapshot(m, eng), before, "dry run")
    assert res["observations"].shape == (T, n_inputs(cfg), M * G)
    for mem in range(M):
        one = to_np(eng.rollout_policy(eng.unflatten_policy(pop[mem], widths, see_pose), T, **layer_kw(cfg, dry_run=True, **LOGS)))
        cols = slice(mem * G, (mem + 1) * G)
        for name in one:
            np.testing.assert_array_equal(res[name][..., cols], one[name][..., cols], err_msg=f"member {mem} {name}")
    S = es_ref.member_sums(res["returns"], M)
    np.testing.assert_array_equal(res["fitness"], es_ref.fitness(S, G))
    assert np.abs(np.diff(res["actions"].reshape(T, -1, M, G)[:, :, :, 0], axis=2)).max() > 0      # the members differ
    assert np.abs(res["reward"]).sum() > 0
    eng.close()


@pytest.mark.parametrize("cfg,tol,auto_reset", [(c, 8.0, False) for c in ALL] + [("min", 30.0, True), ("dh7", 45.0, True)])
def test_committing_call_leaves_what_the_tape_call_leaves_for_its_action_log(m, cfg, tol, auto_reset):
    a = make_engine(m, cfg, tol=tol)
    a.reset_random(SEED, 0)
    a.rollout_population(to_dev(a, host_population(cfg, 1)), 2, **policy_kw(cfg))          # away from the reset state
    state = a.get_state()
    res = to_np(a.rollout_population(to_dev(a, host_population(cfg)), T, **policy_kw(cfg, auto_reset=auto_reset, **LOGS)))
    b = make_engine(m, cfg, tol=tol)
    b.reset_random(SEED + 1, 0)
    b.set_state(state)
    rb = to_np(b.rollout_actions(to_dev(b, res["actions"]), layout="soa", auto_reset=auto_reset, seed=SEED, log=True, returns=True))
    b.sync()
    assert_same(snapshot(m, a), snapshot(m, b), cfg)
    for name in ("reward", "done", "returns"):
        np.testing.assert_array_equal(res[name], rb[name], err_msg=name)
    assert a.bad_action_count() == b.bad_action_count() == 0
    np.testing.assert_array_equal(a.finished(), b.finished())
    if auto_reset:
        assert (a.episodes() > 0).sum() >= 1 and res["done"].sum() >= 1, "no env was re-armed inside the call"
    a.close()
    b.close()


def test_nan_row_holds_that_members_envs_only(m):
    cfg = "six"
    _, M, G = CONFIGS[cfg][:3]
    eng = make_engine(m, cfg)
    eng.reset_random(SEED, 0)
    pop = np.array(host_population(cfg))
    pop[3, 0] = np.uint32(0xFFC00000).view(np.float32)                   # W0[0][0] of member 3
    res = to_np(eng.rollout_population(to_dev(eng, pop), 2, **policy_kw(cfg, actions=True)))
    eng.sync()
    mine = np.zeros(M * G, dtype=bool)
    mine[3 * G:4 * G] = True
    assert np.isnan(res["actions"][:, :, mine]).all() and not np.isnan(res["actions"][:, :, ~mine]).any()
    assert eng.bad_action_count() == 2 * G
    goals = eng.goals()
    assert not goals[mine].any() and goals[~mine].any(axis=1).all()
    eng.close()


# ---- 3. M copies of one policy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ALL)
def test_identical_rows_are_rollout_policy(m, cfg):
    _, M, G, widths, _, _, see_pose = CONFIGS[cfg]
    a, b = make_engine(m, cfg), make_engine(m, cfg)
    for e in (a, b):
        e.reset_random(SEED, 0)
    theta = to_dev(a, host_theta(cfg))
    ra = to_np(a.rollout_population(theta.repeat(M, 1), T, **policy_kw(cfg, **LOGS)))
    rb = to_np(b.rollout_policy(b.unflatten_policy(theta, widths, see_pose), T, **layer_kw(cfg, **LOGS)))
    for name in rb:
        np.testing.assert_array_equal(ra[name], rb[name], err_msg=name)
    assert_same(snapshot(m, a), snapshot(m, b), cfg)
    # sigma so small that sigma * eps adds nothing to any theta_i that is not tiny: the same through sample_population
    big = theta.abs() > 1e-4
    pop = a.sample_population(theta, 1e-13, members=M, seed=SEED)
    assert bool((pop[:, big] == theta[big]).all())
    a.close()
    b.close()


# ---- 4. the generation ----------------------------------------------------------------------------------------------------
def expected_update(cfg, returns, theta, draw, shaping, lr=None):
    _, M, G = CONFIGS[cfg][:3]
    S = es_ref.member_sums(returns, M)
    grad, _ = es_ref.gradient(S, SIGMA, G, draw, SEED, theta.size, shaping)
    out = dict(fitness=es_ref.fitness(S, G), best=np.array([es_ref.best(S)], dtype=np.int32), coeff=es_ref.coefficients(S, shaping),
               sums=S, grad=grad)
    if lr is not None:
        out["theta"] = es_ref.apply(theta, grad, lr)
    return out


@pytest.mark.parametrize("cfg,shaping", [(c, s) for c in ALL for s in ("rank", "raw")])
def test_es_is_sample_score_update(m, cfg, shaping):
    _, M, G = CONFIGS[cfg][:3]
    draw, lr = 2, 0.5
    eng = make_engine(m, cfg)
    eng.reset_random(SEED, 0)
    theta = to_dev(eng, host_theta(cfg))
    scored = to_np(eng.rollout_population(to_dev(eng, host_population(cfg, draw)), T, **policy_kw(cfg, dry_run=True, log=True, returns=True)))
    res = to_np(eng.es(theta, SIGMA, members=M, steps=T, shaping=shaping, draw=draw, log=True, **policy_kw(cfg)))
    np.testing.assert_array_equal(res["population"], host_population(cfg, draw))
    for name in ("returns", "reward", "done"):
        np.testing.assert_array_equal(res[name], scored[name], err_msg=name)
    want = expected_update(cfg, scored["returns"], host_theta(cfg), draw, shaping, lr)
    for name in ("fitness", "best", "sums", "coeff", "grad"):
        np.testing.assert_array_equal(res[name], want[name], err_msg=name)
    assert np.abs(res["grad"]).max() > 0
    np.testing.assert_array_equal(theta.cpu().numpy(), host_theta(cfg))          # not in place: theta is read only
    # in place, from the same state: the same gradient, and theta moved by lr * grad
    eng.reset_random(SEED, 0)
    again = to_np(eng.es(theta, SIGMA, members=M, steps=T, shaping=shaping, draw=draw, lr=lr, inplace=True, **policy_kw(cfg)))
    np.testing.assert_array_equal(again["grad"], want["grad"])
    np.testing.assert_array_equal(theta.cpu().numpy(), want["theta"])
    assert np.any(want["theta"] != host_theta(cfg))
    eng.close()


@pytest.mark.parametrize("shaping", ["rank", "raw"])
def test_ties_take_mid_ranks_and_the_lowest_best(m, shaping):
    """The update on returns written by hand (update_only): members 0, 2 and 5 tie for the largest sum, 1 and 4 further
    down; within member 2 the envs differ, only the sum counts."""
    cfg = "six"
    _, M, G = CONFIGS[cfg][:3]
    eng = make_engine(m, cfg)
    eng.reset_random(SEED, 0)
    before = snapshot(m, eng)
    theta = to_dev(eng, host_theta(cfg))
    per_env = np.repeat(np.array([3, 1, 3, -2, 1, 3], dtype=np.float32), G)
    per_env[2 * G] += 5
    per_env[2 * G + 1] -= 5
    res = to_np(eng.es(theta, SIGMA, members=M, steps=T, shaping=shaping, draw=4, returns=to_dev(eng, per_env), update_only=True,
                       **policy_kw(cfg)))
    eng.sync()
    want = expected_update(cfg, per_env, host_theta(cfg), 4, shaping)
    for name in ("fitness", "best", "sums", "coeff", "grad"):
        np.testing.assert_array_equal(res[name], want[name], err_msg=name)
    assert int(res["best"][0]) == 0
    if shaping == "rank":
        np.testing.assert_array_equal(es_ref.mid_ranks(es_ref.member_sums(per_env, M)), [8, 3, 8, 0, 3, 8])
        np.testing.assert_array_equal(res["coeff"], [5, 8, -5])
    np.testing.assert_array_equal(res["returns"], per_env)
    assert_same(snapshot(m, eng), before, "update only")
    # all sums equal: no direction
    flat = to_np(eng.es(theta, SIGMA, members=M, steps=T, shaping=shaping, draw=4, returns=to_dev(eng, np.full(M * G, -2, np.float32)),
                        update_only=True, lr=1.0, inplace=True, **policy_kw(cfg)))
    assert not flat["grad"].any() and not flat["coeff"].any() and int(flat["best"][0]) == 0
    np.testing.assert_array_equal(theta.cpu().numpy(), host_theta(cfg))
    eng.close()


def test_identical_members_give_a_zero_gradient_through_the_whole_call(m):
    """sigma * eps below half an ulp of every theta_i (theta large): the members are one policy, and with the targets tiled
    over the members they score alike."""
    cfg = "min"
    _, M, G = CONFIGS[cfg][:3]
    eng = make_engine(m, cfg)
    pts = px.sample_targets(SEED, np.arange(G, dtype=np.uint64), 0, K, 51.3)
    eng.reset(np.tile(pts, (M, 1, 1)))
    theta = to_dev(eng, np.where(host_theta(cfg) >= 0, 1.0, -1.0).astype(np.float32) + host_theta(cfg))
    res = to_np(eng.es(theta, 1e-12, members=M, steps=T, **policy_kw(cfg)))
    np.testing.assert_array_equal(res["population"], np.tile(theta.cpu().numpy(), (M, 1)))
    assert res["fitness"][0] == res["fitness"][1] and not res["grad"].any() and int(res["best"][0]) == 0
    eng.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def _raw_es(m, eng, cfg, bufs, **over):
    _, M, G, widths, _, _, see_pose = CONFIGS[cfg]
    arg = m.lib.MtEs()
    arg.struct_size = C.sizeof(m.lib.MtEs)
    arg.shaping, arg.sigma, arg.lr, arg.draw, arg.flags = m.lib.ES_SHAPE_RANK, SIGMA, 0.5, 0, m.lib.ES_INPLACE
    arg.theta, arg.grad_out = bufs["theta"].data_ptr(), bufs["grad"].data_ptr()
    arg.best_out, arg.coeff_out = bufs["best"].data_ptr(), bufs["coeff"].data_ptr()
    p = arg.pop
    p.struct_size, p.n_steps, p.n_members, p.n_layers = C.sizeof(m.lib.MtPopulation), T, M, len(widths) + 1
    for l, w in enumerate(widths):
        p.width[l] = w
    p.hidden_act = m.lib.ACT_RELU if CONFIGS[cfg][4] == "relu" else m.lib.ACT_TANH
    p.out_act = m.lib.ACT_TANH if CONFIGS[cfg][5] == "tanh" else m.lib.ACT_IDENTITY
    p.pop, p.pitch = bufs["pop"].data_ptr(), bufs["pop"].stride(0)
    p.out_scale, p.lo, p.hi = 180.0, -180.0, 180.0
    p.flags = m.lib.POLICY_SEE_POSE if see_pose else 0
    p.return_out, p.fitness_out, p.seed = bufs["returns"].data_ptr(), bufs["fitness"].data_ptr(), SEED
    for name, v in over.items():
        if name.startswith("pop_"):
            setattr(p, name[4:], v)
        else:
            setattr(arg, name, v)
    return arg


def _buffers(eng, cfg, n=None):
    import torch
    _, M, G = CONFIGS[cfg][:3]
    theta = to_dev(eng, host_theta(cfg))
    dev, P = theta.device, theta.numel()
    fill = lambda shape, dtype=torch.float32: torch.full(shape, 9, dtype=dtype, device=dev)      # noqa: E731
    return dict(theta=theta, grad=fill((P,)), best=fill((1,), torch.int32), coeff=fill((M // 2 + M,), torch.int64),
                pop=fill((M, P)), returns=fill((eng.n_envs,)), fitness=fill((M,)))


def test_refusals_name_the_rule_and_touch_nothing(m):
    import torch
    cfg = "six"
    _, M, G = CONFIGS[cfg][:3]
    eng = make_engine(m, cfg)
    bufs = _buffers(eng, cfg)
    P = bufs["theta"].numel()
    INV = m.lib.MT_ERR_INVALID_ARG

    def call(e, arg):
        rc = e._lib.mt_es(e._h, C.byref(arg))
        return rc, e._lib.mt_last_error(e._h).decode()

    rc, msg = call(eng, _raw_es(m, eng, cfg, bufs))
    assert rc == m.lib.MT_ERR_STATE and "before mt_reset" in msg
    eng.reset_random(SEED, 0)
    before = snapshot(m, eng)
    for over, word in [
        (dict(pop_n_members=5), "even"), (dict(pop_n_members=0), "even"), (dict(pop_n_members=8), "n_members"),      # 3072 / 8 = 384
        (dict(pop_n_members=4098), "n_members"), (dict(pop_n_members=3072 // 4), "multiple of 256"),
        (dict(sigma=0.0), "sigma"), (dict(sigma=-1.0), "sigma"), (dict(sigma=float("nan")), "sigma"), (dict(sigma=float("inf")), "sigma"),
        (dict(lr=float("nan")), "lr"), (dict(pop_pitch=P - 1), "pitch"),
        (dict(pop_flags=m.lib.POLICY_DRY_RUN | m.lib.POLICY_AUTO_RESET), "MT_POLICY_DRY_RUN"), (dict(pop_flags=0x8), "flags"),
        (dict(flags=0x4), "MT_ES"), (dict(shaping=2), "shaping"), (dict(reserved=1), "reserved"), (dict(pop_reserved=1), "reserved"),
        (dict(struct_size=8), "struct_size"), (dict(pop_struct_size=8), "struct_size"),
        (dict(pop_n_steps=-1), "n_steps"), (dict(pop_width0=0), "width[0]"), (dict(pop_n_layers=4), "n_layers"),
        (dict(theta=None), "theta"), (dict(coeff_out=None), "coeff_out"), (dict(pop_return_out=None), "return_out"),
        (dict(pop_pop=None), "weight"), (dict(grad_out=bufs["theta"].data_ptr()), "overlaps"),
        (dict(pop_lo=10.0, pop_hi=-10.0), "lo"),
    ]:
        if "pop_width0" in over:
            arg = _raw_es(m, eng, cfg, bufs)
            arg.pop.width[0] = 0
        else:
            arg = _raw_es(m, eng, cfg, bufs, **over)
        rc, msg = call(eng, arg)
        assert rc == INV and word in msg, (over, rc, msg)
    # the parts on their own: the same rules
    s = m.lib.MtEsSample()
    s.struct_size, s.n_members, s.n_params = C.sizeof(m.lib.MtEsSample), M, P
    s.theta, s.pop, s.pitch, s.sigma, s.seed = bufs["theta"].data_ptr(), bufs["pop"].data_ptr(), P, SIGMA, SEED
    for name, v, word in (("n_members", 3, "even"), ("sigma", 0.0, "sigma"), ("pitch", P - 1, "pitch"), ("n_params", 0, "n_params"),
                          ("pop", bufs["theta"].data_ptr(), "overlaps"), ("reserved", 1, "reserved")):
        keep = getattr(s, name)
        setattr(s, name, v)
        assert eng._lib.mt_es_sample(eng._h, C.byref(s)) == INV and word in eng._lib.mt_last_error(eng._h).decode(), name
        setattr(s, name, keep)
    pa = _raw_es(m, eng, cfg, bufs).pop
    for name, v, word in (("n_members", 5, "even"), ("n_members", 8, "n_members"), ("pitch", P - 1, "pitch"),
                          ("flags", m.lib.POLICY_DRY_RUN | m.lib.POLICY_AUTO_RESET, "MT_POLICY_DRY_RUN"), ("return_out", None, "fitness_out")):
        keep = getattr(pa, name)
        setattr(pa, name, v)
        assert eng._lib.mt_rollout_population(eng._h, C.byref(pa)) == INV and word in eng._lib.mt_last_error(eng._h).decode(), name
        setattr(pa, name, keep)
    eng.sync()
    torch.cuda.synchronize()
    assert_same(snapshot(m, eng), before, "refused calls")
    np.testing.assert_array_equal(bufs["theta"].cpu().numpy(), host_theta(cfg))
    for name in ("grad", "best", "coeff", "pop", "returns", "fitness"):
        assert bool((bufs[name] == 9).all()), name
    rc, _ = call(eng, _raw_es(m, eng, cfg, bufs, pop_n_steps=0))         # a no-op
    assert rc == m.lib.MT_OK
    assert_same(snapshot(m, eng), before, "n_steps == 0")
    assert bool((bufs["pop"] == 9).all())
    eng.close()
    # a batch that is no whole number of members, or whose members are no whole blocks
    odd = make_engine(m, "min", n=600)
    odd.reset_random(SEED, 0)
    ob = _buffers(odd, "min")
    for members, word in ((16, "n_members must divide"), (2, "multiple of 256")):          # 600 / 16 = 37.5; 600 / 2 = 300
        rc, msg = call(odd, _raw_es(m, odd, "min", ob, pop_n_members=members))
        assert rc == INV and word in msg, (members, msg)
    odd.close()


def test_python_refusals(m):
    cfg = "min"
    _, M, G = CONFIGS[cfg][:3]
    eng = make_engine(m, cfg)
    eng.reset_random(SEED, 0)
    theta = to_dev(eng, host_theta(cfg))
    pop = to_dev(eng, host_population(cfg))
    kw = policy_kw(cfg)
    with pytest.raises(ValueError, match="even"):
        eng.sample_population(theta, SIGMA, members=3)
    with pytest.raises(ValueError, match="sigma"):
        eng.sample_population(theta, 0.0, members=M)
    with pytest.raises(ValueError, match="sigma"):
        eng.es(theta, float("nan"), members=M, steps=T, **kw)
    with pytest.raises(ValueError, match="dry_run"):
        eng.rollout_population(pop, T, dry_run=True, auto_reset=True, **kw)
    with pytest.raises(ValueError, match="smaller than P"):
        eng.rollout_population(pop[:, :-1], T, **kw)
    with pytest.raises(ValueError, match="multiple of 256"):
        eng.es(theta, SIGMA, members=4, steps=T, **kw)
    with pytest.raises(ValueError, match="P = "):
        eng.es(theta[:-1].contiguous(), SIGMA, members=M, steps=T, **kw)
    with pytest.raises(ValueError, match="shaping"):
        eng.es(theta, SIGMA, members=M, steps=T, shaping="z", **kw)
    with pytest.raises(ValueError, match="lr"):
        eng.es(theta, SIGMA, members=M, steps=T, inplace=True, **kw)
    layers = eng.unflatten_policy(theta, CONFIGS[cfg][3], CONFIGS[cfg][6])
    np.testing.assert_array_equal(eng.flatten_policy(layers).cpu().numpy(), host_theta(cfg))
    assert layers[0][0].data_ptr() == theta.data_ptr()                   # views, not copies
    eng.close()


# ---- 6. stream capture ------------------------------------------------------------------------------------------------
def test_es_call_is_capturable_in_a_hip_graph(m):
    import torch
    cfg = "six"
    _, M, G = CONFIGS[cfg][:3]
    eager, graphed = make_engine(m, cfg), make_engine(m, cfg)
    for e in (eager, graphed):
        e.use_torch_stream()
        e.reset_random(SEED, 0)
    dev = torch.device("cuda", graphed.device)
    bufs = _buffers(graphed, cfg)
    arg = _raw_es(m, graphed, cfg, bufs, flags=0, draw=6)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        graphed.use_torch_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = graphed._lib.mt_es(graphed._h, C.byref(arg))
    assert rc == m.lib.MT_OK, graphed._lib.mt_last_error(graphed._h)
    torch.cuda.synchronize(dev)
    theta = to_dev(eager, host_theta(cfg))
    first = None
    for r in range(2):
        for e in (eager, graphed):
            e.reset_random(SEED, 0)
        torch.cuda.synchronize(dev)
        want = to_np(eager.es(theta, SIGMA, members=M, steps=T, draw=6, **policy_kw(cfg)))
        graph.replay()
        torch.cuda.synchronize(dev)
        got = {"grad": bufs["grad"], "fitness": bufs["fitness"], "best": bufs["best"], "coeff": bufs["coeff"][:M // 2],
               "sums": bufs["coeff"][M // 2:], "population": bufs["pop"], "returns": bufs["returns"]}
        got = to_np(got)
        for name in got:
            np.testing.assert_array_equal(got[name], want[name], err_msg=f"replay {r} {name}")
        assert_same(snapshot(m, graphed), snapshot(m, eager), f"replay {r}")
        if first is None:
            first = got
        else:
            for name in got:
                np.testing.assert_array_equal(got[name], first[name], err_msg=f"replay 0 against 1: {name}")
        for t in bufs.values():
            if t is not bufs["theta"]:
                t.fill_(9)
    assert graphed.goals().any()
    eager.close()
    graphed.close()


# ---- 7. the loop closes -------------------------------------------------------------------------------------------------
def test_ten_generations_follow_the_restatement(m):
    """No learning-curve claim: after every generation theta on the device is the restatement's theta, the returns it is
    fed being those of an evaluation of the restatement's own population (rollout_population, dry run) on the same state."""
    n, M, widths, sigma, lr = 4096, 16, (8,), 0.02, 0.05
    G = n // M
    table, radius = _table(m, "ref")
    eng = m.StepEngine(n, K, dh_table=table, radius=radius, return_ring=RING)
    P = eng.policy_size(widths)
    assert P == (3 * K) * 8 + 8 + 8 * 4 + 4
    layers = policy_ref.make_weights(SEED, 3 * K, widths, 4)
    ref_theta = np.concatenate([t.reshape(-1) for pair in layers for t in pair]).astype(np.float32)
    theta = to_dev(eng, ref_theta)
    kw = dict(widths=widths, hidden="tanh", out="tanh", seed=SEED)
    ids = np.arange(G, dtype=np.uint64)
    means = []
    for gen in range(10):
        eng.reset(np.tile(px.sample_targets(SEED, ids, gen, K, radius), (M, 1, 1)))      # common scenes: the caller's choice
        ref_pop = es_ref.sample_population(ref_theta, sigma, M, gen, SEED)
        scored = to_np(eng.rollout_population(to_dev(eng, ref_pop), T, dry_run=True, returns=True, **kw))
        S = es_ref.member_sums(scored["returns"], M)
        grad, _ = es_ref.gradient(S, sigma, G, gen, SEED, P, "rank")
        ref_theta = es_ref.apply(ref_theta, grad, lr)
        res = to_np(eng.es(theta, sigma, members=M, steps=T, draw=gen, lr=lr, inplace=True, **kw))
        np.testing.assert_array_equal(res["population"], ref_pop, err_msg=f"generation {gen}")
        np.testing.assert_array_equal(res["returns"], scored["returns"], err_msg=f"generation {gen}")
        np.testing.assert_array_equal(res["grad"], grad, err_msg=f"generation {gen}")
        np.testing.assert_array_equal(theta.cpu().numpy(), ref_theta, err_msg=f"generation {gen}")
        means.append(float(res["fitness"].mean()))
    print("mean fitness per generation:", " ".join(f"{v:.3f}" for v in means))
    eng.close()


def test_multienv_evolve_policy_is_es(m):
    n, M = 512, 2
    envs, twin = m.Multienv((1, n), K, rng="device", seed=SEED), m.Multienv((1, n), K, rng="device", seed=SEED)
    envs.reset()
    twin.reset()
    eng = envs._engine
    theta = to_dev(eng, host_theta("min"))
    got = to_np(envs.evolve_policy(theta, SIGMA, M, T, seed=SEED))
    want = to_np(twin._engine.es(theta, SIGMA, members=M, steps=T, seed=SEED))
    for name in want:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    np.testing.assert_array_equal(eng.goals(), twin._engine.goals())
    envs.close()
    twin.close()
