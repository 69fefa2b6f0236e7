"""mt_rollout_actor_critic / StepEngine.rollout_policy(logp=, critic=) / Multienv.collect_policy: the policy rollout that
also writes log pi(a | x), the critic's V(x) per step and V(x_T), in the same launch.

Held to the calls it replaces, bit for bit: rollout_policy without the new keywords on a twin engine for everything
resident and every log; policy_eval on the logs for logp; values on the logs for the values; values on x_T (the
observation a following dry one-step call logs, and observe()'s rows) for last_value.  One configuration per arm is also
held to fp64 (policy_ref.mlp at ac_ref.VALUE_TOL for the values; ac_ref.logp on the mean read back, bit for bit, as
tests/test_gpu_policy_eval.py does).

Arms (n_envs): the reference 4-joint arm, K = 7 (300: a full block and a partial wave); the 7-joint arm, K = 2 (70); a
3-joint runtime table with see_pose, K = 3 (257).  T = 6.  (policy, critic) widths put both register extents and 1, 2, 3
layers on each side, and the extent 64 forced by the critic alone and by the policy alone.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ac_ref
import policy_ref
import staged_populations as sp

pytestmark = pytest.mark.gpu

SEED = 0xAC71
RING = 8
T = 6
SIGMA = 30.0

#         table  K  n    see_pose  pickup_tol that ends episodes inside T steps under sigma = 90
ARMS = {
    "ref": ("ref", 7, 300, False, 45.0),
    "dh7": ("dh7", 2, 70, False, 60.0),
    "rt3": ("rt3", 3, 257, True, 30.0),
}
WIDTHS = (((), (5,)), ((32, 17), (8,)), ((8,), (64, 33)), ((64,), (64, 64)), ((40, 40), ()))
HIDDEN = ("tanh", "relu")
C_OUT = (("identity", 1.0), ("tanh", 2.5))


def _case(ia, iw):
    """(arm, widths index, policy hidden, critic hidden, critic out, critic out_scale): the activations alternate so that
    every arm and every width pair sees both hidden activations and both critic outputs."""
    hidden = HIDDEN[(ia + iw) % 2]
    c_out, c_scale = C_OUT[(ia + (iw + 1) // 2) % 2]
    return (sorted(ARMS)[ia], iw, hidden, HIDDEN[(ia + iw + 1) % 2], c_out, c_scale)


CASES = [_case(ia, iw) for ia in range(len(ARMS)) for iw in range(len(WIDTHS))]
assert {c[2] for c in CASES} == set(HIDDEN) and {c[4] for c in CASES} == {"identity", "tanh"}
IDS = [f"{c[0]}-w{c[1]}-{c[2]}-{c[4]}" for c in CASES]


def case_of(arm, iw):
    return next(c for c in CASES if c[0] == arm and c[1] == iw)


FP64_CASES = [next(c for c in CASES if c[0] == arm and c[4] == "identity" and c[1] in (1, 2, 3)) for arm in sorted(ARMS)]

STATE = ("F_GOALS", "F_POINTS", "F_ALIVE", "F_TOTAL_REWARD", "F_EPISODES", "F_LAST_RETURN", "F_RETURN_RING")
OUTPUTS = ("F_ACTIONS", "F_OBS", "F_REWARD", "F_DONE", "F_DONE_BITS", "F_EE", "F_ZMIN")
LOGS = ("reward", "done", "actions", "observations", "returns")


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def _table(m, name):
    if name == "ref":
        return np.asarray(m.REF_DH_TABLE, dtype=np.float64), 51.3
    if name == "dh7":
        return np.asarray(m.DH7_TABLE, dtype=np.float64), 92.6
    table, _ = sp.fractional_offset_table()
    return np.asarray(table, dtype=np.float64)[:3], 20.0


def make_engine(m, arm, n=None, tol=8.0, k=None, **kw):
    name, K, N, _, _ = ARMS[arm]
    table, radius = _table(m, name)
    return m.StepEngine(N if n is None else n, K if k is None else k, dh_table=table, radius=radius, pickup_tol=tol,
                        return_ring=RING, debug_zmin=True, specialize=(name != "rt3"), **kw)


def n_inputs(arm, dof, k=None):
    return 3 * (ARMS[arm][1] if k is None else k) + (dof if ARMS[arm][3] else 0)


@functools.lru_cache(maxsize=None)
def host_nets(arm, iw, dof, k=None):
    """(policy layers, critic layers) as read-only numpy; the critic is policy_ref's recipe with one output (the weights
    ac_ref.VALUE_TOL was measured on)."""
    pw, cw = WIDTHS[iw]
    n_in = n_inputs(arm, dof, k)
    pol = policy_ref.make_weights(SEED + 7 * iw + len(arm), n_in, pw, dof)
    cri = policy_ref.make_weights(SEED + 7 * iw + len(arm) + 1000, n_in, cw, 1)
    for w, b in pol + cri:
        w.setflags(write=False)
        b.setflags(write=False)
    return tuple(pol), tuple(cri)


def to_dev(eng, layers):
    import torch
    dev = torch.device("cuda", eng.device)
    return [(torch.from_numpy(np.array(w)).to(dev), torch.from_numpy(np.array(b)).to(dev)) for w, b in layers]


def to_np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def snapshot(m, eng):
    snap = {f: eng.get(getattr(m.lib, f)) for f in STATE + OUTPUTS}
    snap.update({"state." + k: np.asarray(v) for k, v in eng.get_state().items()})
    snap["ring"], snap["last_return"], snap["episodes"] = eng.return_ring(), eng.last_return(), eng.episodes()
    snap["bad"] = np.array(eng.bad_action_count())
    return snap


def assert_same(got, want, what=""):
    assert got.keys() == want.keys()
    for f in want:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what} {f}")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def call_kw(case, **over):
    arm, _, hidden = case[:3]
    kw = dict(hidden=hidden, out="tanh", see_pose=ARMS[arm][3], seed=SEED, draw=3)
    kw.update(over)
    return kw


def critic_kw(case):
    return dict(critic_hidden=case[3], critic_out=case[4], critic_out_scale=case[5])


def values_kw(case):
    return dict(hidden=case[3], out=case[4], out_scale=case[5], see_pose=ARMS[case[0]][3])


VARIANTS = {"plain": (False, SIGMA, True), "rearm": (True, 90.0, True), "det": (False, None, False)}


@functools.lru_cache(maxsize=None)
def pair(case, variant):
    """Twin engines from the same seed: A runs rollout_policy with every log, B the same with critic= (and logp=True where
    the variant has a sigma).  -> everything the tests compare, as numpy: both snapshots and result dicts, and on B's logs
    what the replaced calls give (policy_eval's logp, values, values of x_T from a dry one-step call and from observe())."""
    import manytor_amd as m
    import torch
    arm, iw = case[:2]
    auto_reset, sigma, logp = VARIANTS[variant]
    tol = ARMS[arm][4] if auto_reset else 8.0
    a, b = make_engine(m, arm, tol=tol), make_engine(m, arm, tol=tol)
    pol, cri = host_nets(arm, iw, a.dof)
    out = {}
    kw = call_kw(case, sigma=sigma, auto_reset=auto_reset, log=True, returns=True, actions=True, observations=True)
    for name, eng in (("a", a), ("b", b)):
        eng.reset_random(SEED, 0)
        layers, critic = to_dev(eng, pol), to_dev(eng, cri)
        extra = dict(critic=critic, logp=logp, **critic_kw(case)) if name == "b" else {}
        out[name] = to_np(eng.rollout_policy(layers, T, **kw, **extra))
        eng.sync()
        out["snap_" + name] = snapshot(m, eng)
    obs, act = (torch.from_numpy(out["b"][k]).to(torch.device("cuda", b.device)) for k in ("observations", "actions"))
    ekw = dict(hidden=case[2], out="tanh", see_pose=ARMS[arm][3])
    if logp:
        ev = b.policy_eval(layers, obs, actions=act, sigma=sigma, mean=True, **ekw)
        out["eval_logp"], out["eval_mean"] = ev["logp"].cpu().numpy(), ev["mean"].cpu().numpy()
    out["eval_values"] = b.values(critic, obs, **values_kw(case)).cpu().numpy()
    dry = b.rollout_policy(layers, 1, dry_run=True, observations=True, **call_kw(case))
    out["xT"] = dry["observations"].cpu().numpy()[0]
    out["last_from_dry"] = b.values(critic, dry["observations"], **values_kw(case))[0].cpu().numpy()
    if not ARMS[arm][3]:
        b.observe()
        out["last_from_observe"] = b.values(critic, b.device_tensor(m.lib.F_OBS)[None], **values_kw(case))[0].cpu().numpy()
    out["sigma"] = sigma
    a.close()
    b.close()
    return out


def finished_inside(res):
    """(share of envs that finished an episode inside the call, the set of steps at which an env first finished)"""
    done = res["done"] != 0
    first = np.where(done.any(axis=0), done.argmax(axis=0), -1)
    return done.any(axis=0).mean(), set(first[first >= 0].tolist())


# ---- 1. twin ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "rearm"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_resident_state_and_logs_are_rollout_policys(case, variant, m):
    r = pair(case, variant)
    assert_same(r["snap_b"], r["snap_a"], f"{case} {variant}")
    for name in LOGS:
        np.testing.assert_array_equal(r["b"][name], r["a"][name], err_msg=name)
    assert r["b"]["logp"].shape == (T, ARMS[case[0]][2]) and r["b"]["last_value"].shape == (ARMS[case[0]][2],)
    assert np.abs(np.diff(r["a"]["actions"], axis=0)).max() > 0
    if variant == "rearm":
        share, steps = finished_inside(r["a"])
        print(f"{case[0]}: {share:.3f} of the envs finished inside the call, first at steps {sorted(steps)}")
        assert share >= 0.05 and len(steps) > 1, (share, steps)
        assert (r["snap_a"]["episodes"] > 0).any()


@pytest.mark.parametrize("case", [c for c in CASES if c[1] == 1], ids=[i for c, i in zip(CASES, IDS) if c[1] == 1])
def test_critic_alone_with_a_deterministic_policy(case, m):
    r = pair(case, "det")
    assert_same(r["snap_b"], r["snap_a"], f"{case} det")
    for name in LOGS:
        np.testing.assert_array_equal(r["b"][name], r["a"][name], err_msg=name)
    assert "logp" not in r["b"]
    np.testing.assert_array_equal(bits(r["b"]["values"]), bits(r["eval_values"]))
    np.testing.assert_array_equal(bits(r["b"]["last_value"]), bits(r["last_from_dry"]))


# ---- 2. logp ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "rearm"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_logp_is_policy_evals_on_the_logs(case, variant, m):
    r = pair(case, variant)
    assert np.abs(r["eval_logp"]).max() > 0
    np.testing.assert_array_equal(bits(r["b"]["logp"]), bits(r["eval_logp"]))


@pytest.mark.parametrize("case", [c for c in CASES if c[1] in (0, 3)], ids=[i for c, i in zip(CASES, IDS) if c[1] in (0, 3)])
def test_logp_needs_neither_log(case, m):
    r = pair(case, "plain")
    arm, iw = case[:2]
    eng = make_engine(m, arm)
    eng.reset_random(SEED, 0)
    pol, cri = host_nets(arm, iw, eng.dof)
    res = eng.rollout_policy(to_dev(eng, pol), T, logp=True, critic=to_dev(eng, cri), **critic_kw(case),
                             **call_kw(case, sigma=SIGMA, observations=False, actions=False))
    assert sorted(res) == ["last_value", "logp", "values"]
    got = to_np(res)
    for name in ("logp", "values", "last_value"):
        np.testing.assert_array_equal(bits(got[name]), bits(r["b"][name]), err_msg=name)
    only = to_np(eng.rollout_policy(to_dev(eng, pol), T, logp=True, dry_run=True, **call_kw(case, sigma=SIGMA)))
    assert sorted(only) == ["logp"] and only["logp"].shape == (T, ARMS[arm][2])
    eng.close()


# ---- 3. values ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "rearm"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_values_are_values_on_the_logs(case, variant, m):
    r = pair(case, variant)
    assert np.ptp(r["eval_values"]) > 0
    np.testing.assert_array_equal(bits(r["b"]["values"]), bits(r["eval_values"]))


# ---- 4. last_value ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "rearm"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_last_value_is_the_critic_on_the_state_behind_the_last_step(case, variant, m):
    r = pair(case, variant)
    np.testing.assert_array_equal(bits(r["b"]["last_value"]), bits(r["last_from_dry"]))
    if not ARMS[case[0]][3]:
        np.testing.assert_array_equal(bits(r["b"]["last_value"]), bits(r["last_from_observe"]))


def test_last_value_behind_a_re_arm_in_the_last_step(m):
    hits = 0
    for case in CASES:
        r = pair(case, "rearm")
        ended = r["a"]["done"][T - 1] != 0
        if not ended.any():
            continue
        hits += 1
        arm = case[0]
        if ARMS[arm][3]:                                                 # the pose x_T shows is the zero pose
            assert not r["xT"][3 * ARMS[arm][1]:, ended].any()
        np.testing.assert_array_equal(bits(r["b"]["last_value"][ended]), bits(r["last_from_dry"][ended]))
    assert hits, "no case ended an episode in the last step"


# ---- 5. fp64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FP64_CASES, ids=[c[0] for c in FP64_CASES])
def test_values_and_logp_against_fp64(case, m):
    r = pair(case, "plain")
    arm, iw = case[:2]
    dof = r["a"]["actions"].shape[1]
    _, cri = host_nets(arm, iw, dof)
    obs = r["b"]["observations"]
    n = obs.shape[-1]
    x = obs.transpose(1, 0, 2).reshape(obs.shape[1], T * n)
    v64 = policy_ref.mlp(x, cri, case[3], case[4], case[5])[0].reshape(T, n)
    err = np.abs(r["b"]["values"] - v64).max()
    print(f"{arm}: max |V - V_fp64| = {err:.3e} (gate {ac_ref.VALUE_TOL:.3e})")
    assert err <= ac_ref.VALUE_TOL
    x_t = r["xT"]
    l64 = policy_ref.mlp(x_t, cri, case[3], case[4], case[5])[0]
    assert np.abs(r["b"]["last_value"] - l64).max() <= ac_ref.VALUE_TOL
    want = ac_ref.logp(r["eval_mean"], r["b"]["actions"], r["sigma"])
    np.testing.assert_array_equal(bits(r["b"]["logp"]), bits(want))


# ---- 6. unusable actions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [case_of("ref", 1), case_of("dh7", 3), case_of("rt3", 2)], ids=["ref", "dh7", "rt3"])
def test_unusable_actions_get_logp_zero_and_their_values(case, m):
    import torch
    arm, iw = case[:2]
    a, b = make_engine(m, arm), make_engine(m, arm)
    pol, cri = host_nets(arm, iw, a.dof)
    a.reset_random(SEED, 0)
    probe = a.rollout_policy(to_dev(a, pol), 1, dry_run=True, actions=True, **call_kw(case, out="identity", out_scale=1.0))
    reach = np.abs(probe["actions"].cpu().numpy()[0]).max(axis=0)
    scale = 32768.0 / float(np.percentile(reach, 75))                   # a quarter of the envs leave the range at step 0
    kw = call_kw(case, out="identity", out_scale=scale, sigma=SIGMA, log=True, returns=True, actions=True, observations=True)
    ra = to_np(a.rollout_policy(to_dev(a, pol), T, **kw))
    b.reset_random(SEED, 0)
    layers, critic = to_dev(b, pol), to_dev(b, cri)
    rb = to_np(b.rollout_policy(layers, T, logp=True, critic=critic, **critic_kw(case), **kw))
    bad = (np.abs(rb["actions"]) > 32768.0).any(axis=1)
    assert 0 < bad.sum() < bad.size
    assert (rb["logp"][bad] == 0).all() and (bits(rb["logp"][bad]) == 0).all()
    assert (rb["logp"][~bad] != 0).any()
    dev = torch.device("cuda", b.device)
    obs, act = torch.from_numpy(rb["observations"]).to(dev), torch.from_numpy(rb["actions"]).to(dev)
    lp = b.policy_eval(layers, obs, actions=act, sigma=SIGMA, mean=False, hidden=case[2], out="identity", out_scale=scale,
                       see_pose=ARMS[arm][3])["logp"].cpu().numpy()
    np.testing.assert_array_equal(bits(rb["logp"]), bits(lp))
    np.testing.assert_array_equal(bits(rb["values"]), bits(b.values(critic, obs, **values_kw(case)).cpu().numpy()))
    assert_same(snapshot(m, b), snapshot(m, a), "unusable")
    assert b.bad_action_count() == int(bad.sum())
    for name in LOGS:
        np.testing.assert_array_equal(rb[name], ra[name], err_msg=name)
    a.close()
    b.close()


# ---- 7. dry run ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[2], CASES[9], CASES[13]], ids=[IDS[2], IDS[9], IDS[13]])
def test_dry_run_changes_nothing_resident_and_writes_the_same_outputs(case, m):
    r = pair(case, "plain")
    arm, iw = case[:2]
    eng = make_engine(m, arm)
    eng.reset_random(SEED, 0)
    eng.sync()
    pol, cri = host_nets(arm, iw, eng.dof)
    before = snapshot(m, eng)
    res = to_np(eng.rollout_policy(to_dev(eng, pol), T, dry_run=True, logp=True, critic=to_dev(eng, cri), **critic_kw(case),
                                   **call_kw(case, sigma=SIGMA, log=True, returns=True, actions=True, observations=True)))
    assert_same(snapshot(m, eng), before, "dry run")
    for name in LOGS + ("logp", "values", "last_value"):
        np.testing.assert_array_equal(bits(res[name]) if res[name].dtype == np.float32 else res[name],
                                      bits(r["b"][name]) if res[name].dtype == np.float32 else r["b"][name], err_msg=name)
    eng.close()


# ---- the raw struct -----------------------------------------------------------------------------------------------------
def raw_arg(m, eng, case, layers, critic, steps=T, sigma=SIGMA, **over):
    L = m.lib
    full = L.MtActorCritic()
    full.struct_size = C.sizeof(L.MtActorCritic)
    p = full.policy
    p.struct_size, p.n_steps, p.n_layers = C.sizeof(L.MtPolicy), steps, len(layers)
    acts = {"tanh": L.ACT_TANH, "relu": L.ACT_RELU, "identity": L.ACT_IDENTITY}
    for l, (w, b) in enumerate(layers):
        p.weight[l], p.bias[l] = w.data_ptr(), b.data_ptr()
        if l < len(layers) - 1:
            p.width[l] = int(w.shape[0])
    p.hidden_act, p.out_act = acts[case[2]], L.ACT_TANH
    p.out_scale, p.lo, p.hi, p.seed, p.draw = 180.0, -180.0, 180.0, SEED, 3
    p.flags = L.POLICY_SEE_POSE if ARMS[case[0]][3] else 0
    p.sigma[:] = [sigma] * eng.dof + [0.0] * (L.MT_MAX_DOF - eng.dof)
    for l, (w, b) in enumerate(critic):
        full.critic_weight[l], full.critic_bias[l] = w.data_ptr(), b.data_ptr()
        if l < len(critic) - 1:
            full.critic_width[l] = int(w.shape[0])
    full.critic_layers = len(critic)
    full.critic_hidden_act, full.critic_out_act, full.critic_out_scale = acts[case[3]], acts[case[4]], case[5]
    for name, v in over.items():
        if name.startswith("policy_"):
            setattr(p, name[7:], v)
        else:
            setattr(full, name, v)
    return full


def raw_call(eng, full):
    rc = eng._lib.mt_rollout_actor_critic(eng._h, C.byref(full))
    return rc, eng._lib.mt_last_error(eng._h).decode()


# ---- 8. pad columns -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[0], CASES[7], CASES[14]], ids=[IDS[0], IDS[7], IDS[14]])
def test_pad_columns_keep_their_contents(case, m):
    import torch
    r = pair(case, "plain")
    arm, iw = case[:2]
    eng = make_engine(m, arm)
    eng.use_torch_stream()
    eng.reset_random(SEED, 0)
    n, d = eng.n_envs, eng.dof
    ld, IN = n + 37, n_inputs(arm, eng.dof)
    dev = torch.device("cuda", eng.device)
    pol, cri = host_nets(arm, iw, d)
    layers, critic = to_dev(eng, pol), to_dev(eng, cri)
    fill = lambda rows, dtype=torch.float32: torch.full((rows, ld), 77, dtype=dtype, device=dev)      # noqa: E731
    logp, val, act, obs = fill(T), fill(T), fill(T * d), fill(T * IN)
    rew, done, last = fill(T, torch.int8), fill(T, torch.uint8), fill(1)
    full = raw_arg(m, eng, case, layers, critic, logp_log=logp.data_ptr(), logp_ld=ld, value_log=val.data_ptr(), value_ld=ld,
                   last_value_out=last.data_ptr(), policy_action_log=act.data_ptr(), policy_act_ld=ld,
                   policy_obs_log=obs.data_ptr(), policy_obs_ld=ld, policy_reward_log=rew.data_ptr(),
                   policy_done_log=done.data_ptr(), policy_log_ld=ld)
    rc, msg = raw_call(eng, full)
    assert rc == m.lib.MT_OK, msg
    torch.cuda.synchronize(dev)
    for buf, name, rows in ((logp, "logp", None), (val, "values", None), (act, "actions", d), (obs, "observations", IN),
                            (rew, "reward", None), (done, "done", None)):
        got = buf.cpu().numpy()
        assert (got[:, n:] == 77).all(), name
        want = r["b"][name].reshape(got.shape[0], n)
        np.testing.assert_array_equal(bits(got[:, :n]) if got.dtype == np.float32 else got[:, :n],
                                      bits(want) if got.dtype == np.float32 else want, err_msg=name)
    got = last.cpu().numpy()[0]
    assert (got[n:] == 77).all()
    np.testing.assert_array_equal(bits(got[:n]), bits(r["b"]["last_value"]))
    eng.close()


# ---- 9. capture ---------------------------------------------------------------------------------------------------------
def test_call_is_capturable_in_a_hip_graph(m):
    import torch
    case = CASES[3]
    arm, iw = case[:2]
    eager, graphed = make_engine(m, arm), make_engine(m, arm)
    for e in (eager, graphed):
        e.use_torch_stream()
        e.reset_random(SEED, 0)
    dev = torch.device("cuda", graphed.device)
    n = graphed.n_envs
    pol, cri = host_nets(arm, iw, graphed.dof)
    layers, critic = to_dev(graphed, pol), to_dev(graphed, cri)
    logp, val = (torch.zeros((T, n), dtype=torch.float32, device=dev) for _ in range(2))
    last = torch.zeros((n,), dtype=torch.float32, device=dev)
    full = raw_arg(m, graphed, case, layers, critic, logp_log=logp.data_ptr(), logp_ld=n, value_log=val.data_ptr(), value_ld=n,
                   last_value_out=last.data_ptr())
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        graphed.use_torch_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = graphed._lib.mt_rollout_actor_critic(graphed._h, C.byref(full))
    assert rc == m.lib.MT_OK, graphed._lib.mt_last_error(graphed._h)
    torch.cuda.synchronize(dev)
    graphed.reset_random(SEED, 0)         # the capture pass itself does not execute; start from the same state anyway
    torch.cuda.synchronize(dev)
    for rep in range(2):
        want = to_np(eager.rollout_policy(layers, T, logp=True, critic=critic, **critic_kw(case), **call_kw(case, sigma=SIGMA)))
        graph.replay()
        torch.cuda.synchronize(dev)
        for buf, name in ((logp, "logp"), (val, "values"), (last, "last_value")):
            np.testing.assert_array_equal(bits(buf.cpu().numpy()), bits(want[name]), err_msg=f"replay {rep} {name}")
        assert_same(snapshot(m, graphed), snapshot(m, eager), f"replay {rep}")
    assert graphed.goals().any()
    eager.close()
    graphed.close()


# ---- 10. shards ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[4], CASES[6], CASES[12]], ids=[IDS[4], IDS[6], IDS[12]])
def test_a_shard_computes_the_whole_batchs_columns(case, m):
    r = pair(case, "plain")
    arm, iw = case[:2]
    n = ARMS[arm][2]
    half = n // 2
    eng = make_engine(m, arm, n=n - half, env_id_base=half)
    eng.reset_random(SEED, 0)
    pol, cri = host_nets(arm, iw, eng.dof)
    got = to_np(eng.rollout_policy(to_dev(eng, pol), T, logp=True, critic=to_dev(eng, cri), **critic_kw(case),
                                   **call_kw(case, sigma=SIGMA)))
    for name in ("logp", "values", "last_value"):
        np.testing.assert_array_equal(bits(got[name]), bits(r["b"][name][..., half:]), err_msg=name)
    eng.close()


# ---- 11. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field_and_change_nothing(m):
    import torch
    case = case_of("ref", 1)
    arm, iw = case[:2]
    eng = make_engine(m, arm)
    eng.use_torch_stream()
    eng.reset_random(SEED, 0)
    n, d = eng.n_envs, eng.dof
    dev = torch.device("cuda", eng.device)
    pol, cri = host_nets(arm, iw, d)
    layers, critic = to_dev(eng, pol), to_dev(eng, cri)

    def roomy(t):
        """`t` at the front of a buffer as long as a log: an output that starts at it reaches no other allocation"""
        big = torch.zeros(t.numel() + T * n, dtype=torch.float32, device=dev)
        big[:t.numel()] = t.reshape(-1)
        return big[:t.numel()].view(t.shape)

    critic[0] = (roomy(critic[0][0]), critic[0][1])
    layers[1] = (layers[1][0], roomy(layers[1][1]))
    logp, val = (torch.zeros((T, n), dtype=torch.float32, device=dev) for _ in range(2))
    act = torch.zeros((T, d, n), dtype=torch.float32, device=dev)
    last = torch.zeros((n,), dtype=torch.float32, device=dev)
    base = dict(logp_log=logp.data_ptr(), logp_ld=n, value_log=val.data_ptr(), value_ld=n, last_value_out=last.data_ptr(),
                policy_action_log=act.data_ptr(), policy_act_ld=n)
    torch.cuda.synchronize(dev)
    before = snapshot(m, eng)

    def refused(word, status=None, sigma=SIGMA, **over):
        rc, msg = raw_call(eng, raw_arg(m, eng, case, layers, critic, sigma=sigma, **dict(base, **over)))
        assert rc == (m.lib.MT_ERR_INVALID_ARG if status is None else status), (rc, msg)
        assert word in msg, msg

    full = raw_arg(m, eng, case, layers, critic, **base)
    full.policy.sigma[d - 1] = 0.0
    rc, msg = raw_call(eng, full)
    assert rc == m.lib.MT_ERR_INVALID_ARG and f"sigma[{d - 1}]" in msg, msg
    refused("value_log overlaps critic_weight / critic_bias [0]", value_log=critic[0][0].data_ptr())
    refused("logp_log overlaps weight / bias [1]", logp_log=layers[1][1].data_ptr())
    refused("logp_log overlaps policy.action_log", logp_log=act.data_ptr() + 4 * n)
    refused("value_log overlaps last_value_out", last_value_out=val.data_ptr() + 4 * n * (T - 1))
    refused("logp_ld", logp_ld=n - 1)
    refused("value_ld", value_ld=n - 1)
    refused("policy.act_ld", policy_act_ld=n - 1)
    refused("critic_weight / critic_bias [2] is NULL", critic_layers=3, critic_width=(C.c_int32 * 2)(8, 8))
    torch.cuda.synchronize(dev)
    assert_same(snapshot(m, eng), before, "refusals")
    assert not logp.cpu().numpy().any() and not val.cpu().numpy().any() and not last.cpu().numpy().any()

    # Python-side: the critic's shape, by layer
    kw = call_kw(case, sigma=SIGMA)
    w0, b0 = critic[0]
    two = [critic[0], (torch.zeros((2, 8), device=dev), torch.zeros(2, device=dev))]
    with pytest.raises(ValueError, match=r"critic layer 1: weight must be \(1, 8\)"):
        eng.rollout_policy(layers, T, critic=two, **kw)
    with pytest.raises(ValueError, match=r"critic layer 0: weight must be \(8, %d\)" % n_inputs(arm, d)):
        eng.rollout_policy(layers, T, critic=[(torch.zeros((8, 5), device=dev), b0), critic[1]], **kw)
    wide = torch.zeros((8, 2 * n_inputs(arm, d)), device=dev)[:, ::2]
    with pytest.raises(ValueError, match="critic layer 0: weight must be a contiguous"):
        eng.rollout_policy(layers, T, critic=[(wide, b0), critic[1]], **kw)
    with pytest.raises(ValueError, match="logp needs sigma"):
        eng.rollout_policy(layers, T, logp=True, **call_kw(case))
    with pytest.raises(ValueError, match="critic_out must be"):
        eng.rollout_policy(layers, T, critic=critic, critic_out="relu", **kw)
    assert_same(snapshot(m, eng), before, "python refusals")
    eng.close()


def test_a_critic_on_a_handle_whose_targets_and_input_exceed_the_lds_is_unsupported(m):
    """3 K + IN <= 160: K = 27 asks for 162 rows of 256 floats.  logp alone has no such limit."""
    arm, iw, k = "ref", 0, 27
    case = case_of(arm, iw)
    eng = make_engine(m, arm, n=64, k=k)
    eng.reset_random(SEED, 0)
    eng.sync()
    pol, cri = host_nets(arm, iw, eng.dof, k)
    before = snapshot(m, eng)
    with pytest.raises(m.lib.ManytorError, match="3 K \\+ IN <= 160") as err:
        eng.rollout_policy(to_dev(eng, pol), 2, critic=to_dev(eng, cri), **critic_kw(case), **call_kw(case))
    assert err.value.status == m.lib.MT_ERR_UNSUPPORTED
    assert_same(snapshot(m, eng), before, "unsupported")
    res = eng.rollout_policy(to_dev(eng, pol), 2, logp=True, **call_kw(case, sigma=SIGMA))
    assert np.isfinite(res["logp"].cpu().numpy()).all()
    eng.close()


def test_the_largest_supported_target_count_runs(m):
    """K = 26 without see_pose: 156 rows, 156 KB of LDS in one block."""
    import torch
    arm, iw, k = "ref", 1, 26
    case = case_of(arm, iw)
    eng = make_engine(m, arm, n=300, k=k)
    eng.reset_random(SEED, 0)
    pol, cri = host_nets(arm, iw, eng.dof, k)
    layers, critic = to_dev(eng, pol), to_dev(eng, cri)
    res = eng.rollout_policy(layers, 3, logp=True, critic=critic, observations=True, **critic_kw(case), **call_kw(case, sigma=SIGMA))
    want = eng.values(critic, res["observations"], **values_kw(case))
    np.testing.assert_array_equal(bits(res["values"].cpu().numpy()), bits(want.cpu().numpy()))
    eng.close()


# ---- 12. Multienv -------------------------------------------------------------------------------------------------------
def test_multienv_collect_policy_is_the_engines_call(m):
    case = case_of("ref", 0)
    arm, iw = case[:2]
    r = pair(case, "plain")
    envs = m.Multienv((1, ARMS[arm][2]), ARMS[arm][1], return_ring=RING)
    eng = envs._engine
    eng.reset_random(SEED, 0)
    pol, cri = host_nets(arm, iw, eng.dof)
    idx = envs._step_idx
    res = envs.collect_policy(to_dev(eng, pol), T, logp=True, critic=to_dev(eng, cri), log=True, **critic_kw(case),
                              **call_kw(case, sigma=SIGMA))
    assert envs._step_idx == idx + T
    got = to_np(res)
    assert sorted(got) == ["done", "last_value", "logp", "reward", "values"]
    for name in got:
        np.testing.assert_array_equal(got[name], r["b"][name], err_msg=name)
    envs.collect_policy(to_dev(eng, pol), T, logp=True, dry_run=True, **call_kw(case, sigma=SIGMA))
    assert envs._step_idx == idx + T


# ---- 13. zero steps -----------------------------------------------------------------------------------------------------
def test_zero_steps_is_a_no_op(m):
    import torch
    case = CASES[1]
    arm, iw = case[:2]
    eng = make_engine(m, arm)
    eng.use_torch_stream()
    eng.reset_random(SEED, 0)
    n = eng.n_envs
    dev = torch.device("cuda", eng.device)
    pol, cri = host_nets(arm, iw, eng.dof)
    layers, critic = to_dev(eng, pol), to_dev(eng, cri)
    logp, val = (torch.full((T, n), 77.0, device=dev) for _ in range(2))
    last = torch.full((n,), 77.0, device=dev)
    torch.cuda.synchronize(dev)
    before = snapshot(m, eng)
    rc, msg = raw_call(eng, raw_arg(m, eng, case, layers, critic, steps=0, logp_log=logp.data_ptr(), logp_ld=n,
                                    value_log=val.data_ptr(), value_ld=n, last_value_out=last.data_ptr()))
    assert rc == m.lib.MT_OK, msg
    torch.cuda.synchronize(dev)
    assert (logp.cpu().numpy() == 77).all() and (val.cpu().numpy() == 77).all() and (last.cpu().numpy() == 77).all()
    assert_same(snapshot(m, eng), before, "zero steps")
    res = eng.rollout_policy(layers, 0, logp=True, critic=critic, **critic_kw(case), **call_kw(case, sigma=SIGMA))
    assert res["logp"].shape == (0, n) and res["values"].shape == (0, n) and res["last_value"].shape == (n,)
    assert_same(snapshot(m, eng), before, "zero steps, python")
    eng.close()
