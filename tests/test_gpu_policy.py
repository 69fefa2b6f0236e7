"""mt_rollout_policy / StepEngine.rollout_policy / Multienv.run_policy: T x (observe; MLP; step) in one launch.

Held to three references:
  * mt_rollout_tape on a twin engine, fed the call's own action log: every resident field, the last step's outputs, the
    logs, returns, ring and counters, bit for bit (the environment semantics are DEFINED by that call);
  * the fp64 oracle's observation of the twin's state in front of every step (parity_util.assert_obs_close: the project's
    gates) for what the policy saw;
  * tests/policy_ref.py -- an fp64 MLP on the kernel's own fp32 input, the tag-4 noise stream, the clamp rule -- for the
    action, within ACTION_TOL_DEG.
Shapes: 300 envs (a partial wave and a partial second block), 6 steps (3 at K = 32).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import policy_ref
import staged_populations as sp
from oracle import manytor_oracle as mo
from parity_util import assert_obs_close

pytestmark = pytest.mark.gpu

SEED = 0x90C1
RING = 8
N = 300

#            table  K   widths    hidden  out         see_pose T
CONFIGS = {
    "ref_k7": ("ref", 7, (32, 32), "tanh", "tanh", False, 6),
    "ref_k1": ("ref", 1, (), "tanh", "tanh", False, 6),
    "ref_k32": ("ref", 32, (64, 64), "relu", "identity", True, 3),     # the largest LDS tile, input and register footprint
    "dh7": ("dh7", 3, (17, 5), "tanh", "tanh", False, 6),              # odd widths below a compiled extent
    "rt5": ("rt5", 3, (32,), "tanh", "tanh", True, 6),                 # a runtime table (specialize=False), two layers
    "narrow": ("ref", 2, (3, 1), "tanh", "tanh", False, 6),            # rows of 3 and of 1 weight: shorter than a block of eight
}
ALL = sorted(CONFIGS)

STATE = ("F_GOALS", "F_POINTS", "F_ALIVE", "F_TOTAL_REWARD", "F_EPISODES", "F_LAST_RETURN", "F_RETURN_RING")
OUTPUTS = ("F_OBS", "F_REWARD", "F_DONE", "F_DONE_BITS", "F_EE", "F_ZMIN")
EVERYTHING = ("F_ACTIONS",) + STATE + OUTPUTS


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
    table, radius = sp.fractional_offset_table()
    return np.asarray(table, dtype=np.float64), radius


def make_engine(m, cfg, n=N, tol=8.0, **kw):
    name, k = CONFIGS[cfg][:2]
    table, radius = _table(m, name)
    return m.StepEngine(n, k, dh_table=table, radius=radius, pickup_tol=tol, return_ring=RING, debug_zmin=True,
                        specialize=(name != "rt5"), **kw)


def n_inputs(cfg, dof):
    return 3 * CONFIGS[cfg][1] + (dof if CONFIGS[cfg][5] else 0)


@functools.lru_cache(maxsize=None)
def host_weights(cfg, dof):
    layers = policy_ref.make_weights(SEED + len(cfg) + CONFIGS[cfg][1], n_inputs(cfg, dof), CONFIGS[cfg][2], dof)
    for w, b in layers:
        w.setflags(write=False)
        b.setflags(write=False)
    return tuple(layers)


def device_weights(eng, layers):
    import torch
    dev = torch.device("cuda", eng.device)
    return [(torch.from_numpy(np.array(w)).to(dev), torch.from_numpy(np.array(b)).to(dev)) for w, b in layers]


def policy_kw(cfg, **over):
    _, _, _, hidden, out, see_pose, _ = CONFIGS[cfg]
    kw = dict(hidden=hidden, out=out, see_pose=see_pose, seed=SEED)
    kw.update(over)
    return kw


def snapshot(m, eng, fields):
    return {f: eng.get(getattr(m.lib, f)) for f in fields}


def assert_same(got, want, what=""):
    assert got.keys() == want.keys()
    for f in want:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what} {f}")


def to_np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def run(m, cfg, *, tol=8.0, T=None, n=N, env_id_base=0, layers=None, **over):
    """A fresh engine of `cfg`, reset, one rollout_policy call with everything logged -> (engine, results as numpy)."""
    eng = make_engine(m, cfg, n=n, tol=tol, env_id_base=env_id_base)
    eng.reset_random(SEED, 0)
    layers = host_weights(cfg, eng.dof) if layers is None else layers
    res = eng.rollout_policy(device_weights(eng, layers), CONFIGS[cfg][6] if T is None else T,
                             **policy_kw(cfg, log=True, returns=True, actions=True, observations=True, **over))
    eng.sync()
    return eng, to_np(res)


# ---- 1. replay identity -----------------------------------------------------------------------------------------------
# auto_reset: one target and a wide pickup box (ref_k1), three targets and tol 45 on the 7-joint arm (dh7), with exploration
# noise that spreads the poses: envs finish inside the T steps and are re-armed there.
@pytest.mark.parametrize("cfg,tol,auto_reset,sigma", [(c, 8.0, False, None) for c in ALL] + [
    ("ref_k1", 20.0, True, 90.0), ("dh7", 45.0, True, 90.0), ("ref_k7", 8.0, False, 30.0)])
def test_policy_call_leaves_what_the_tape_call_leaves_for_its_action_log(m, cfg, tol, auto_reset, sigma):
    a, res = run(m, cfg, tol=tol, auto_reset=auto_reset, sigma=sigma)
    b = make_engine(m, cfg, tol=tol)
    b.reset_random(SEED, 0)
    import torch
    tape = torch.from_numpy(res["actions"]).to(torch.device("cuda", b.device))
    rb = to_np(b.rollout_actions(tape, layout="soa", auto_reset=auto_reset, seed=SEED, log=True, returns=True))
    b.sync()
    assert_same(snapshot(m, a, EVERYTHING), snapshot(m, b, EVERYTHING), cfg)
    for name in ("reward", "done", "returns"):
        np.testing.assert_array_equal(res[name], rb[name], err_msg=name)
    assert a.bad_action_count() == b.bad_action_count() == 0
    np.testing.assert_array_equal(a.finished(), b.finished())
    assert np.abs(np.diff(res["actions"], axis=0)).max() > 0            # the policy reacted to the state
    if auto_reset:
        assert (a.episodes() > 0).sum() >= 1 and res["done"].sum() >= 1, "no env was re-armed inside the call"
    a.close()
    b.close()


# ---- 2. the policy saw the state's observation ---------------------------------------------------------------------
def assert_saw_the_state(twin, cfg, table, obs_t):
    """obs_t (IN, N), what the policy saw in front of a step, against the fp64 observation of the twin's state there."""
    k, see_pose = CONFIGS[cfg][1], CONFIGS[cfg][5]
    goals, points, alive = twin.goals(), twin.points().astype(np.float64), twin.alives().astype(bool)
    elbow = mo.batch_joints_coordinates(goals.astype(np.float64), table)[:, -2]
    want = mo.observe(elbow, points, alive)
    assert_obs_close(np.ascontiguousarray(obs_t[:3 * k].T), want, elbow, points, alive)
    if see_pose:
        np.testing.assert_array_equal(obs_t[3 * k:].T, goals)


@pytest.mark.parametrize("cfg,tol,auto_reset,sigma", [(c, 8.0, False, None) for c in ALL] + [("dh7", 45.0, True, 90.0)])
def test_policy_input_is_the_observation_of_the_state_each_step_starts_from(m, cfg, tol, auto_reset, sigma):
    a, res = run(m, cfg, tol=tol, auto_reset=auto_reset, sigma=sigma)
    name, T = CONFIGS[cfg][0], CONFIGS[cfg][6]
    table, _ = _table(m, name)
    b = make_engine(m, cfg, tol=tol)
    b.reset_random(SEED, 0)
    obs = res["observations"]
    assert obs.shape == (T, n_inputs(cfg, b.dof), N)
    rearmed = 0
    for t in range(T):
        assert_saw_the_state(b, cfg, table, obs[t])
        b.set_actions(np.ascontiguousarray(res["actions"][t].T))
        b.step()
        if auto_reset:
            rearmed += int((b.get(m.lib.F_DONE) != 0).sum())
            b.reset_done(SEED)
    assert not auto_reset or rearmed >= 1
    assert_same(snapshot(m, a, STATE), snapshot(m, b, STATE), cfg)
    a.close()
    b.close()


# ---- 3. the action is the MLP of what it saw -------------------------------------------------------------------------
def expected_actions(cfg, dof, layers, obs, *, sigma=None, draw=0, out_scale=180.0, lo=-180.0, hi=180.0, env_id_base=0, out=None):
    _, _, _, hidden, out_cfg, _, _ = CONFIGS[cfg]
    T, _, n = obs.shape
    want = np.empty((T, dof, n), dtype=np.float64)
    z = policy_ref.policy_noise(SEED, np.arange(n, dtype=np.uint64) + np.uint64(env_id_base), draw, T, dof)
    for t in range(T):
        a64 = policy_ref.mlp(obs[t], layers, hidden, out or out_cfg, out_scale)
        if sigma is not None:
            sg = np.broadcast_to(np.float32(sigma), (dof,)).astype(np.float32)
            a64 = a64 + (sg[:, None] * z[t]).astype(np.float64)
        want[t] = np.clip(a64, lo, hi)
    return want


@pytest.mark.parametrize("cfg,sigma", [(c, None) for c in ALL] + [("ref_k7", 25.0), ("dh7", (0, 5, 10, 0, 20, 40, 80))])
def test_action_is_the_mlp_of_the_logged_observation(m, cfg, sigma):
    a, res = run(m, cfg, sigma=sigma, draw=3)
    want = expected_actions(cfg, a.dof, host_weights(cfg, a.dof), res["observations"], sigma=sigma, draw=3)
    err = np.abs(res["actions"].astype(np.float64) - want)
    print(f"{cfg} sigma={sigma}: max |a_kernel - a_fp64| = {err.max():.3g} deg over {err.size} actions")
    assert err.max() <= policy_ref.ACTION_TOL_DEG
    assert np.abs(res["actions"]).max() <= 180.0
    a.close()


def _first_outputs(m, cfg, **over):
    """(D, N): what the policy of `cfg` puts out at the reset state, unclamped (a one-step dry run with wide bounds)."""
    eng = make_engine(m, cfg)
    eng.reset_random(SEED, 0)
    res = eng.rollout_policy(device_weights(eng, host_weights(cfg, eng.dof)), 1,
                             **policy_kw(cfg, actions=True, dry_run=True, lo=-32768.0, hi=32768.0, **over))
    first = res["actions"].cpu().numpy()[0]
    eng.close()
    return first


def test_outputs_past_lo_hi_are_clamped_exactly(m):
    cfg = "ref_k7"
    first = _first_outputs(m, cfg, out="identity", out_scale=120.0)
    lo, hi = (float(np.float32(v)) for v in np.percentile(first, [30, 70]))     # three in ten leave each side at step 0
    assert hi - lo > 1.0
    a, res = run(m, cfg, out="identity", out_scale=120.0, lo=lo, hi=hi)
    want = expected_actions(cfg, a.dof, host_weights(cfg, a.dof), res["observations"], out="identity", out_scale=120.0, lo=lo, hi=hi)
    act = res["actions"]
    raw = expected_actions(cfg, a.dof, host_weights(cfg, a.dof), res["observations"], out="identity", out_scale=120.0,
                           lo=-32768.0, hi=32768.0)
    inside = (raw > lo + 1e-2) & (raw < hi - 1e-2)
    low, high = raw < lo - 1e-2, raw > hi + 1e-2
    assert low.sum() > 0 and high.sum() > 0 and inside.sum() > 0
    assert np.all(act[low] == np.float32(lo)) and np.all(act[high] == np.float32(hi))
    assert np.abs(act.astype(np.float64) - want).max() <= policy_ref.ACTION_TOL_DEG
    a.close()


def test_tanh_error_is_within_its_constant(m):
    """The kernel's tanh against fp64 tanh on the hidden pre-activations of the populations above: the network with an
    identity output, a unit last layer and out_scale = 1 hands its last hidden vector out (as many units as the arm has
    joints per call; the unit rows walk over the layer)."""
    worst = 0.0
    for cfg in ("ref_k7", "dh7", "rt5"):
        eng = make_engine(m, cfg)
        dof = eng.dof
        layers = list(host_weights(cfg, dof))
        width = layers[-1][0].shape[1]
        for first in range(0, width, dof):
            eng.reset_random(SEED, 0)
            pick = np.zeros((dof, width), dtype=np.float32)
            for j in range(dof):
                pick[j, (first + j) % width] = 1.0
            probe = layers[:-1] + [(pick, np.zeros(dof, dtype=np.float32))]
            res = to_np(eng.rollout_policy(device_weights(eng, probe), 2, **policy_kw(cfg, out="identity", out_scale=1.0, lo=-2.0,
                                                                                      hi=2.0, actions=True, observations=True)))
            for t in range(2):
                pre = []
                policy_ref.mlp(res["observations"][t], probe, "tanh", "identity", 1.0, np.float64, pre)
                want = np.tanh(pre[-1])
                for j in range(dof):
                    worst = max(worst, float(np.abs(res["actions"][t, j] - want[(first + j) % width]).max()))
        eng.close()
    print(f"max |tanh_kernel - tanh_fp64| = {worst:.3g} (includes the rounding of the layers in front of it)")
    assert worst <= policy_ref.TANH_ABS_ERR


# ---- 4. noise ---------------------------------------------------------------------------------------------------------
def test_noise_is_sigma_times_the_tag4_variate(m):
    cfg = "dh7"
    eng = make_engine(m, cfg)
    eng.reset_random(SEED, 0)
    dof = eng.dof
    w = device_weights(eng, host_weights(cfg, dof))
    sigma = np.array([3.0, 0.0, 11.5, 0.25, 40.0, 7.0, 1.0], dtype=np.float32)
    kw = policy_kw(cfg, actions=True, dry_run=True)
    det = to_np(eng.rollout_policy(w, 1, **kw))["actions"][0]
    noisy = to_np(eng.rollout_policy(w, 1, sigma=sigma, draw=9, **kw))["actions"][0]
    other = to_np(eng.rollout_policy(w, 1, sigma=sigma, draw=10, **kw))["actions"][0]
    z = policy_ref.policy_noise(SEED, np.arange(N, dtype=np.uint64), 9, 1, dof)[0]
    sz = sigma[:, None] * z                                             # fp32: one rounding
    free = (np.abs(det) < 180.0) & (np.abs(noisy) < 180.0)              # neither side clamped
    assert free.mean() > 0.5
    diff = noisy.astype(np.float64) - det.astype(np.float64)
    ulp = np.spacing(np.abs(noisy))
    assert np.all(np.abs(diff - sz)[free] <= ulp[free])
    np.testing.assert_array_equal(noisy[1], det[1])                     # sigma_j == 0: no noise on that joint
    assert (other != noisy)[[0, 2, 3, 4, 5, 6]].mean() > 0.9
    assert eng.bad_action_count() == 0 and not eng.goals().any()
    eng.close()


# ---- 5. sharding --------------------------------------------------------------------------------------------------------
def test_shards_compute_what_the_whole_batch_computes(m):
    cfg = "ref_k7"
    whole, rw = run(m, cfg, sigma=20.0, draw=2)
    parts = [run(m, cfg, n=n, env_id_base=base, sigma=20.0, draw=2) for base, n in ((0, 128), (128, 172))]
    for name, axis in (("actions", 2), ("observations", 2), ("reward", 1), ("done", 1), ("returns", 0)):
        np.testing.assert_array_equal(np.concatenate([r[name] for _, r in parts], axis=axis), rw[name], err_msg=name)
    np.testing.assert_array_equal(np.concatenate([e.goals() for e, _ in parts]), whole.goals())
    for e in [whole] + [e for e, _ in parts]:
        e.close()


# ---- 6. dry run --------------------------------------------------------------------------------------------------------
def test_dry_run_changes_nothing_resident(m):
    cfg = "ref_k7"
    eng = make_engine(m, cfg)
    eng.reset_random(SEED, 0)
    w = device_weights(eng, host_weights(cfg, eng.dof))
    eng.rollout_policy(w, 2, **policy_kw(cfg))                           # away from the reset state
    before, version = snapshot(m, eng, EVERYTHING), eng.version
    kw = policy_kw(cfg, sigma=15.0, log=True, returns=True, actions=True, observations=True)
    dry = to_np(eng.rollout_policy(w, 6, dry_run=True, **kw))
    eng.sync()
    assert_same(snapshot(m, eng, EVERYTHING), before, "dry run")
    assert eng.bad_action_count() == 0 and eng.version == version
    real = to_np(eng.rollout_policy(w, 6, **kw))
    for name in real:
        np.testing.assert_array_equal(dry[name], real[name], err_msg=name)
    assert np.abs(real["reward"]).sum() > 0
    with pytest.raises(ValueError, match="dry_run"):
        eng.rollout_policy(w, 1, dry_run=True, auto_reset=True, **policy_kw(cfg))
    eng.close()


# ---- 7. unusable output --------------------------------------------------------------------------------------------------
def test_unusable_output_holds_the_pose_and_is_counted(m):
    """An identity output scaled so that some envs' angles leave +-32768 degrees: such a value is handed on as it is, the env
    holds its pose for that step, the pair is counted, and the step-by-step path agrees about all of it.  The step behind a
    held pose is the one whose observation frame comes from a route that went nowhere: what the policy saw there is held
    to the oracle as well."""
    cfg, T = "ref_k7", 3
    reach = np.abs(_first_outputs(m, cfg, out="identity", out_scale=1.0)).max(axis=0)     # (N,): each env's largest |y| at step 0
    scale = 32768.0 / float(np.percentile(reach, 75))                                     # a quarter of the envs leave the range there
    eng, res = run(m, cfg, T=T, out="identity", out_scale=scale)
    act = res["actions"]
    bad = (np.abs(act) > 32768.0).any(axis=1)                            # (T, N)
    assert 0 < bad.sum() < bad.size and (~bad).all(axis=0).sum() > 0
    assert eng.bad_action_count() == int(bad.sum())
    assert np.abs(act[np.abs(act) <= 32768.0]).max() <= 180.0           # usable values are clamped
    twin = make_engine(m, cfg)
    twin.reset_random(SEED, 0)
    goals = twin.goals()
    table, _ = _table(m, CONFIGS[cfg][0])
    assert (bad[:-1].sum(axis=0) > 0).sum() > 0                          # some env starts a step from a held pose
    for t in range(T):
        assert_saw_the_state(twin, cfg, table, res["observations"][t])
        twin.set_actions(np.ascontiguousarray(act[t].T))
        twin.step()
        now = twin.goals()
        np.testing.assert_array_equal(now[bad[t]], goals[bad[t]])        # held
        np.testing.assert_array_equal(now[~bad[t]], act[t].T[~bad[t]])
        goals = now
    assert_same(snapshot(m, eng, STATE), snapshot(m, twin, STATE), "unusable")
    assert twin.bad_action_count() == int(bad.sum())
    eng.close()
    twin.close()


def test_nan_weight_ends_in_unusable_actions(m):
    """A NaN among the weights of a relu layer (sign bit set: the pattern a sign test would take for a negative number) is
    not swallowed by the activation: every action is NaN, every env holds its pose, every pair is counted."""
    cfg, T = "ref_k32", 2
    layers = [(np.array(w), np.array(b)) for w, b in host_weights(cfg, 4)]
    layers[0][0][:, 0] = np.uint32(0xFFC00000).view(np.float32)
    eng, res = run(m, cfg, T=T, layers=layers)
    assert np.isnan(res["actions"]).all()
    assert eng.bad_action_count() == N * T and not eng.goals().any()
    eng.close()


# ---- 8. stream capture ------------------------------------------------------------------------------------------------
def test_policy_call_is_capturable_in_a_hip_graph(m):
    import torch
    cfg, T = "ref_k7", 4
    eager, graphed = make_engine(m, cfg), make_engine(m, cfg)
    for e in (eager, graphed):
        e.use_torch_stream()
        e.reset_random(SEED, 0)
    dev = torch.device("cuda", graphed.device)
    dof = graphed.dof
    layers = device_weights(graphed, host_weights(cfg, dof))
    act = torch.zeros((T, dof, N), dtype=torch.float32, device=dev)
    ret = torch.zeros((N,), dtype=torch.float32, device=dev)
    arg = m.lib.MtPolicy()
    arg.struct_size, arg.n_steps, arg.n_layers = C.sizeof(m.lib.MtPolicy), T, 3
    arg.width[0], arg.width[1] = 32, 32
    arg.hidden_act = arg.out_act = m.lib.ACT_TANH
    for l, (w, b) in enumerate(layers):
        arg.weight[l], arg.bias[l] = w.data_ptr(), b.data_ptr()
    arg.out_scale, arg.lo, arg.hi = 180.0, -180.0, 180.0
    arg.action_log, arg.act_ld, arg.return_out, arg.seed = act.data_ptr(), N, ret.data_ptr(), SEED
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        graphed.use_torch_stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = graphed._lib.mt_rollout_policy(graphed._h, C.byref(arg))
    assert rc == m.lib.MT_OK, graphed._lib.mt_last_error(graphed._h)
    torch.cuda.synchronize(dev)
    graphed.reset_random(SEED, 0)         # the capture pass itself does not execute; start from the same state anyway
    torch.cuda.synchronize(dev)
    for r in range(2):
        want = eager.rollout_policy(layers, T, **policy_kw(cfg, actions=True, returns=True))
        graph.replay()
        torch.cuda.synchronize(dev)
        np.testing.assert_array_equal(act.cpu().numpy(), want["actions"].cpu().numpy(), err_msg=f"replay {r}")
        np.testing.assert_array_equal(ret.cpu().numpy(), want["returns"].cpu().numpy(), err_msg=f"replay {r}")
        assert_same(snapshot(m, graphed, EVERYTHING), snapshot(m, eager, EVERYTHING), f"replay {r}")
    assert graphed.goals().any()
    eager.close()
    graphed.close()


# ---- 9. refusals -------------------------------------------------------------------------------------------------------
def _raw_policy(m, eng, layers, **over):
    arg = m.lib.MtPolicy()
    arg.struct_size, arg.n_steps, arg.n_layers = C.sizeof(m.lib.MtPolicy), 2, len(layers)
    for l, (w, b) in enumerate(layers):
        arg.weight[l], arg.bias[l] = w.data_ptr(), b.data_ptr()
        if l < len(layers) - 1:
            arg.width[l] = int(w.shape[0])
    arg.hidden_act = arg.out_act = m.lib.ACT_TANH
    arg.out_scale, arg.lo, arg.hi, arg.seed = 180.0, -180.0, 180.0, SEED
    for name, v in over.items():
        if name.startswith("width"):
            arg.width[int(name[5:])] = v
        elif name == "weight1":
            arg.weight[1] = v
        else:
            setattr(arg, name, v)
    return arg


def _refused(m, eng, arg):
    rc = eng._lib.mt_rollout_policy(eng._h, C.byref(arg))
    return rc, eng._lib.mt_last_error(eng._h).decode()


def test_refusals_name_the_field(m):
    import torch
    cfg = "ref_k7"
    eng = make_engine(m, cfg)
    layers = device_weights(eng, host_weights(cfg, eng.dof))
    rc, msg = _refused(m, eng, _raw_policy(m, eng, layers))
    assert rc == m.lib.MT_ERR_STATE and "before mt_reset" in msg
    eng.reset_random(SEED, 0)
    before = snapshot(m, eng, EVERYTHING)
    log = torch.zeros((2, eng.dof, N), dtype=torch.float32, device=layers[0][0].device)
    INV = m.lib.MT_ERR_INVALID_ARG
    for over, status, word in [
        (dict(width0=0), INV, "width[0]"), (dict(width1=65), INV, "width[1]"),
        (dict(n_layers=0), INV, "n_layers"), (dict(n_layers=4), INV, "n_layers"),
        (dict(hidden_act=7), INV, "hidden_act"), (dict(out_act=m.lib.ACT_RELU), INV, "out_act"),
        (dict(hidden_act=m.lib.ACT_IDENTITY), INV, "hidden_act"),
        (dict(flags=m.lib.POLICY_DRY_RUN | m.lib.POLICY_AUTO_RESET), INV, "MT_POLICY_DRY_RUN"),
        (dict(flags=0x8), INV, "flags"), (dict(reserved=1), INV, "reserved"), (dict(struct_size=8), INV, "struct_size"),
        (dict(n_steps=65536), INV, "n_steps"), (dict(n_steps=-1), INV, "n_steps"),
        (dict(weight1=None), INV, "weight"),
        (dict(action_log=log.data_ptr(), act_ld=N - 1), INV, "act_ld"),
        (dict(obs_log=log.data_ptr(), obs_ld=N - 1), INV, "obs_ld"),
        (dict(reward_log=log.data_ptr(), log_ld=N - 1), INV, "log_ld"),
        (dict(lo=float("nan")), INV, "lo"), (dict(lo=10.0, hi=-10.0), INV, "lo"), (dict(out_scale=float("inf")), INV, "out_scale"),
    ]:
        rc, msg = _refused(m, eng, _raw_policy(m, eng, layers, **over))
        assert rc == status and word in msg, (over, rc, msg)
    arg = _raw_policy(m, eng, layers)
    arg.sigma[2] = -1.0
    rc, msg = _refused(m, eng, arg)
    assert rc == INV and "sigma[2]" in msg
    eng.sync()
    assert_same(snapshot(m, eng, EVERYTHING), before, "refused calls")
    rc, _ = _refused(m, eng, _raw_policy(m, eng, layers, n_steps=0))     # a no-op
    assert rc == m.lib.MT_OK
    assert_same(snapshot(m, eng, EVERYTHING), before, "n_steps == 0")
    eng.close()
    table, radius = _table(m, "ref")
    for kw in (dict(trace=True), dict(obs_frame=-3)):
        odd = m.StepEngine(N, 7, dh_table=table, radius=radius, **kw)
        odd.reset_random(SEED, 0)
        rc, msg = _refused(m, odd, _raw_policy(m, odd, layers))
        assert rc == m.lib.MT_ERR_UNSUPPORTED and "mt_rollout_policy" in msg, (kw, rc, msg)
        assert odd.dispatch()["policy_rollout"]["usable"] is False
        odd.close()


def test_python_checks_name_the_layer(m):
    import torch
    cfg = "ref_k7"
    eng = make_engine(m, cfg)
    eng.reset_random(SEED, 0)
    layers = device_weights(eng, host_weights(cfg, eng.dof))
    kw = policy_kw(cfg)
    with pytest.raises(ValueError, match="layer 1"):
        eng.rollout_policy([layers[0], (layers[1][0][:, :-1].contiguous(), layers[1][1]), layers[2]], 1, **kw)
    with pytest.raises(ValueError, match="layer 2.*contiguous float32"):
        eng.rollout_policy([layers[0], layers[1], (layers[2][0].double(), layers[2][1])], 1, **kw)
    with pytest.raises(ValueError, match="layer 0.*contiguous float32"):
        eng.rollout_policy([(layers[0][0].cpu(), layers[0][1]), layers[1], layers[2]], 1, **kw)
    with pytest.raises(ValueError, match="hidden"):
        eng.rollout_policy(layers, 1, **policy_kw(cfg, hidden="gelu"))
    net = torch.nn.Sequential(torch.nn.Linear(21, 32), torch.nn.Tanh(), torch.nn.Linear(32, 32), torch.nn.Tanh(),
                              torch.nn.Linear(32, 4), torch.nn.Tanh()).to(layers[0][0].device)
    with torch.no_grad():
        for lin, (w, b) in zip([net[0], net[2], net[4]], layers):
            lin.weight.copy_(w)
            lin.bias.copy_(b)
    with pytest.raises(ValueError, match="do not agree"):
        eng.rollout_policy(net, 1, **policy_kw(cfg, hidden="relu"))
    got = eng.rollout_policy(net, 3, **policy_kw(cfg, actions=True, dry_run=True))["actions"].cpu().numpy()
    want = eng.rollout_policy(layers, 3, **policy_kw(cfg, actions=True, dry_run=True))["actions"].cpu().numpy()
    np.testing.assert_array_equal(got, want)
    eng.close()


# ---- 10. Multienv.run_policy --------------------------------------------------------------------------------------------
def test_multienv_run_policy_returns_what_the_steps_return(m):
    import torch
    cfg, n, T = "ref_k7", 5, 4
    k = CONFIGS[cfg][1]
    envs, twin = m.Multienv((1, n), k, rng="device", seed=SEED), m.Multienv((1, n), k, rng="device", seed=SEED)
    envs.reset()
    twin.reset()
    eng = envs._engine
    layers = device_weights(eng, host_weights(cfg, eng.dof))
    obs2, rew, done = envs.run_policy(layers, T, **policy_kw(cfg))
    probe = m.Multienv((1, n), k, rng="device", seed=SEED)
    probe.reset()
    acts = probe._engine.rollout_policy(layers, T, **policy_kw(cfg, actions=True))["actions"].cpu().numpy()
    assert isinstance(rew, list) and len(rew) == T and len(rew[0]) == n
    for t in range(T):
        o, r, d = twin.step(np.ascontiguousarray(acts[t].T).tolist())
        assert [int(v) for v in r] == rew[t] and [bool(v) for v in d] == done[t]
    for got, want in zip(obs2, o):
        np.testing.assert_array_equal(np.asarray(got), np.asarray(want))
    for e in (envs, twin, probe):
        e.close()
