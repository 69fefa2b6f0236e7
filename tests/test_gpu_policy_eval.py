"""mt_policy_eval (StepEngine.policy_eval, .values, Multienv.evaluate_policy): the MLP's forward pass over logged
observations -- the mean of every sample and the log-probability of the logged actions under the current weights.

Held to:
  * rollout_policy's own action_log, bit for bit (the mean of a deterministic dry run IS the logged action);
  * policy_ref.mlp in fp64 within policy_ref.ACTION_TOL_DEG (the D-output policy at out_scale 180) and ac_ref.VALUE_TOL (a
    one-output identity head);
  * ac_ref.logp on the mean read back, and policy_grad's loss with a one-hot coef, bit for bit;
  * the unusable-action rule, the bounds of every read and write, determinism (twice, under a HIP graph, across ld's).
Shapes: the families of tests/test_gpu_policy_grad.py::CONFIGS -- one block / several, T = 1 and 3, NaN pad columns, an
n_envs that is no multiple of 64, widths 1 .. 64 (both register extents), K = 32, the 4-joint and the 7-joint arm.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ac_ref
import policy_ref
import test_gpu_policy_grad as base
from test_gpu_policy_grad import dev_layers, dof_of, engine, n_inputs, padded, to_dev

pytestmark = pytest.mark.gpu

SEED = 0xAC71
SIGMA = 20.0
CONFIGS = {k: base.CONFIGS[k] for k in ("one", "two", "pad", "odd", "w1", "w64", "k32")}
ALL = sorted(CONFIGS)


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def shape_kw(cfg):
    return dict(hidden=CONFIGS[cfg][6], see_pose=CONFIGS[cfg][8])


@functools.lru_cache(maxsize=None)
def host_layers(cfg, n_out=None):
    """The config's policy (n_out None: D outputs) or a head with n_out outputs on the same hidden widths."""
    return policy_ref.make_weights(SEED + len(cfg) + (n_out or 0), n_inputs(cfg), CONFIGS[cfg][5], n_out or dof_of(cfg))


_LOGS = {}


def logs(m, cfg, out="tanh"):
    """A DETERMINISTIC dry run of the config's policy (sigma = 0): obs_log and action_log as numpy arrays, computed once.
    out="tanh" at out_scale 180 with lo / hi = -+180: the clamp can never bind.  out="identity" at out_scale 20."""
    if (cfg, out) not in _LOGS:
        eng = engine(m, cfg)
        eng.reset_random(SEED, 0)
        res = eng.rollout_policy(dev_layers(eng, host_layers(cfg)), CONFIGS[cfg][3], sigma=0, seed=SEED, out=out,
                                 out_scale=180.0 if out == "tanh" else 20.0, lo=-180.0, hi=180.0, actions=True, observations=True,
                                 dry_run=True, **shape_kw(cfg))
        eng.sync()
        got = {k: v.cpu().numpy() for k, v in res.items()}
        for v in got.values():
            v.setflags(write=False)
        _LOGS[cfg, out] = got
    return _LOGS[cfg, out]


def noisy_actions(cfg, mean):
    """Actions of the logs' shape around `mean`, a few sigma away: what a noisy rollout would have logged."""
    rng = np.random.RandomState(SEED % 1000 + len(cfg))
    return (mean + SIGMA * rng.randn(*mean.shape)).astype(np.float32)


def run(m, cfg, obs, actions=None, ld=None, fill=np.nan, layers=None, **over):
    """policy_eval on [..., :n] views of (..., ld) buffers with `fill` in the pad columns -> dict of numpy arrays."""
    eng = engine(m, cfg)
    ld = CONFIGS[cfg][2] if ld is None else ld
    kw = dict(out="tanh", out_scale=180.0, **shape_kw(cfg))
    kw.update(over)
    if actions is not None:
        kw.update(actions=padded(eng, actions, ld, fill), sigma=kw.pop("sigma", SIGMA))
    res = eng.policy_eval(dev_layers(eng, host_layers(cfg)) if layers is None else layers, padded(eng, obs, ld, fill), **kw)
    eng.sync()
    return {k: v.cpu().numpy() for k, v in res.items()}


def flat(a):
    """(T, rows, n) -> (rows, T n): the samples side by side, as policy_ref.mlp takes them."""
    return np.moveaxis(a, 0, -2).reshape(a.shape[1], -1)


# ---- 1. the mean is rollout_policy's action, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("cfg", ALL)
def test_mean_is_rollout_policys_action_bit_for_bit(m, cfg):
    data = logs(m, cfg)
    got = run(m, cfg, data["observations"])["mean"]
    assert got.shape == data["actions"].shape and np.isfinite(got).all() and np.abs(got).max() > 0
    np.testing.assert_array_equal(got.view(np.uint32), data["actions"].view(np.uint32))


@pytest.mark.parametrize("cfg", ALL)
def test_identity_mean_is_rollout_policys_action_inside_the_clamp(m, cfg):
    data = logs(m, cfg, "identity")
    got = run(m, cfg, data["observations"], out="identity", out_scale=20.0)["mean"]
    inside = (data["actions"] > -180.0) & (data["actions"] < 180.0)
    assert inside.mean() >= 0.9, inside.mean()
    np.testing.assert_array_equal(got[inside].view(np.uint32), data["actions"][inside].view(np.uint32))
    assert (np.abs(got[~inside]) >= 180.0).all()                 # what the clamp caught lies outside


# ---- 2. against fp64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ALL)
def test_mean_against_fp64(m, cfg):
    data = logs(m, cfg)
    got = flat(run(m, cfg, data["observations"])["mean"])
    want = policy_ref.mlp(flat(data["observations"]), host_layers(cfg), CONFIGS[cfg][6], "tanh", 180.0)
    err = float(np.abs(got - want).max())
    print(f"policy_eval {cfg}: max |mean - fp64| = {err:.3e} degrees")
    assert err <= policy_ref.ACTION_TOL_DEG


def value_errors(m, cfg):
    """(max |V - V64|, max |V32 - V64|) of the config's one-output identity head at out_scale 1 on its logged observations."""
    eng = engine(m, cfg)
    obs = logs(m, cfg)["observations"]
    head = host_layers(cfg, 1)
    got = eng.values(dev_layers(eng, head), to_dev(eng, obs), **shape_kw(cfg))
    eng.sync()
    got = got.cpu().numpy()
    assert got.shape == (obs.shape[0], obs.shape[2])
    v64 = policy_ref.mlp(flat(obs), head, CONFIGS[cfg][6], "identity", 1.0)[0]
    v32 = policy_ref.mlp(flat(obs), head, CONFIGS[cfg][6], "identity", 1.0, dtype=np.float32)[0]
    return float(np.abs(got.reshape(-1) - v64).max()), float(np.abs(v32 - v64).max())


@pytest.mark.parametrize("cfg", ALL)
def test_value_head_against_fp64(m, cfg):
    err, err32 = value_errors(m, cfg)
    print(f"policy_eval {cfg}: one-output identity head max |V - fp64| = {err:.3e} (numpy fp32 restatement {err32:.3e})")
    assert ac_ref.VALUE_TOL <= 16.0 * ac_ref.VALUE_REF32_MEASURED
    assert err <= ac_ref.VALUE_TOL, (err, ac_ref.VALUE_TOL)


def test_n_out_one_and_n_out_d_on_the_same_handle(m):
    cfg = "odd"
    eng = engine(m, cfg)
    obs = logs(m, cfg)["observations"]
    head = dev_layers(eng, host_layers(cfg, 1))
    first = run(m, cfg, obs)["mean"]
    v = run(m, cfg, obs, layers=head, n_out=1, out="identity", out_scale=1.0)["mean"]
    again = run(m, cfg, obs)["mean"]
    assert v.shape == (obs.shape[0], 1, obs.shape[2])
    np.testing.assert_array_equal(again, first)
    np.testing.assert_array_equal(first, logs(m, cfg)["actions"])
    v64 = policy_ref.mlp(flat(obs), host_layers(cfg, 1), CONFIGS[cfg][6], "identity", 1.0)
    assert np.abs(flat(v) - v64).max() <= ac_ref.VALUE_TOL
    with pytest.raises(ValueError):                              # the D-output layers are no one-output head
        eng.policy_eval(dev_layers(eng, host_layers(cfg)), to_dev(eng, obs), n_out=1, **shape_kw(cfg))


# ---- 3. logp ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ALL)
def test_logp_is_the_stated_sequence_on_the_mean_read_back(m, cfg):
    data = logs(m, cfg)
    act = noisy_actions(cfg, data["actions"])
    sigma = np.linspace(5.0, 30.0, dof_of(cfg)).astype(np.float32)
    got = run(m, cfg, data["observations"], act, sigma=sigma)
    np.testing.assert_array_equal(got["mean"], data["actions"])
    want = ac_ref.logp(got["mean"], act, sigma)
    assert (want < 0).all()
    np.testing.assert_array_equal(got["logp"].view(np.uint32), want.view(np.uint32))
    only = run(m, cfg, data["observations"], act, sigma=sigma, mean=False)
    assert sorted(only) == ["logp"]
    np.testing.assert_array_equal(only["logp"], got["logp"])


@pytest.mark.parametrize("cfg", ALL)
def test_logp_is_policy_grads_loss_with_a_one_hot_coef(m, cfg):
    import torch
    eng = engine(m, cfg)
    data = logs(m, cfg)
    _, n, _, T = CONFIGS[cfg][:4]
    act = noisy_actions(cfg, data["actions"])
    layers = dev_layers(eng, host_layers(cfg))
    obs_d, act_d = to_dev(eng, data["observations"]), to_dev(eng, act)
    kw = dict(out="tanh", out_scale=180.0, **shape_kw(cfg))
    lp = eng.policy_eval(layers, obs_d, actions=act_d, sigma=SIGMA, mean=False, **kw)["logp"]
    eng.sync()
    lp = lp.cpu().numpy()
    for t, i in ((0, 0), (T - 1, n - 1), (T // 2, n // 2 + 1)):
        coef = torch.zeros((T, n), dtype=torch.float32, device=obs_d.device)
        coef[t, i] = 1.0
        _, loss = eng.policy_grad(layers, obs_d, act_d, coef, sigma=SIGMA, scale=1.0, loss=True, **kw)
        eng.sync()
        assert np.float32(loss.cpu().numpy()[0]) == lp[t, i] and lp[t, i] < 0, (t, i)


@pytest.mark.parametrize("cfg", ["two", "pad", "odd"])
def test_unusable_actions_give_logp_zero_and_change_nothing_else(m, cfg):
    data = logs(m, cfg)
    act = noisy_actions(cfg, data["actions"])
    clean = run(m, cfg, data["observations"], act)
    rng = np.random.RandomState(3)
    T, d, n = act.shape
    hit = rng.rand(T, n) < 0.2
    bad = np.array(act)
    poison = np.array([np.nan, np.inf, -np.inf, 40000.0], dtype=np.float32)
    for t, i in zip(*np.nonzero(hit)):
        bad[t, rng.randint(d), i] = poison[rng.randint(4)]
    got = run(m, cfg, data["observations"], bad)
    assert hit.any() and (got["logp"][hit] == 0).all()
    np.testing.assert_array_equal(got["logp"][~hit].view(np.uint32), clean["logp"][~hit].view(np.uint32))
    np.testing.assert_array_equal(got["mean"], clean["mean"])    # mu does not depend on the action
    np.testing.assert_array_equal(got["logp"], ac_ref.logp(got["mean"], bad, SIGMA))


# ---- 4. bounds, the ld's, determinism -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["pad", "odd", "w1", "w64"])
def test_pad_columns_are_neither_read_nor_written_whatever_the_ld(m, cfg):
    import torch
    eng = engine(m, cfg)
    dev = torch.device("cuda", eng.device)
    data = logs(m, cfg)
    act = noisy_actions(cfg, data["actions"])
    T, d, n = act.shape
    first = run(m, cfg, data["observations"], act)
    again = run(m, cfg, data["observations"], act)
    for k in first:
        np.testing.assert_array_equal(again[k].view(np.uint32), first[k].view(np.uint32))
    for ld, fill in ((n, 0.0), (n + 1000, -np.inf)):
        got = run(m, cfg, data["observations"], act, ld=ld, fill=fill)
        for k in first:
            np.testing.assert_array_equal(got[k].view(np.uint32), first[k].view(np.uint32), err_msg=f"{k} at ld {ld}")
    # every matrix and vector inside NaN, 3 words of it on each side; sentinel pad columns and rows around both outputs
    layers = []
    for w, b in host_layers(cfg):
        pair = []
        for a in (w, b):
            buf = torch.full((a.size + 6,), float("nan"), dtype=torch.float32, device=dev)
            buf[3:3 + a.size] = to_dev(eng, a.reshape(-1))
            pair.append(buf[3:3 + a.size].view(a.shape))
        layers.append(tuple(pair))
    ld = CONFIGS[cfg][2] + 5
    mean_buf = torch.full((T * d + 2, ld), -123.25, dtype=torch.float32, device=dev)
    logp_buf = torch.full((T + 2, ld + 2), -123.25, dtype=torch.float32, device=dev)
    mean_out = mean_buf[1:T * d + 1].view(T, d, ld)[..., :n]
    logp_out = logp_buf[1:T + 1, :n]
    got = run(m, cfg, data["observations"], act, ld=ld, layers=layers, mean=mean_out, logp=logp_out)
    for k in first:
        np.testing.assert_array_equal(got[k].view(np.uint32), first[k].view(np.uint32), err_msg=k)
    mb, lb = mean_buf.cpu().numpy(), logp_buf.cpu().numpy()
    assert (mb[0] == -123.25).all() and (mb[-1] == -123.25).all() and (mb[:, n:] == -123.25).all()
    assert (lb[0] == -123.25).all() and (lb[-1] == -123.25).all() and (lb[:, n:] == -123.25).all()
    assert (first["mean"] != -123.25).all() and (first["logp"] != -123.25).all()


def test_call_is_capturable_in_a_hip_graph(m):
    import torch
    cfg = "pad"
    eng = engine(m, cfg)
    data = logs(m, cfg)
    act = noisy_actions(cfg, data["actions"])
    want = run(m, cfg, data["observations"], act)
    dev = torch.device("cuda", eng.device)
    ld = CONFIGS[cfg][2]
    layers = dev_layers(eng, host_layers(cfg))
    obs_d, act_d = padded(eng, data["observations"], ld), padded(eng, act, ld)
    mean_out, logp_out = torch.zeros(want["mean"].shape, device=dev), torch.zeros(want["logp"].shape, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    try:
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                eng.policy_eval(layers, obs_d, actions=act_d, sigma=SIGMA, mean=mean_out, logp=logp_out, out="tanh", **shape_kw(cfg))
        torch.cuda.synchronize(dev)
        assert not mean_out.cpu().numpy().any()                  # captured, not run
        for r in range(2):
            mean_out.fill_(3.0)
            logp_out.fill_(3.0)
            graph.replay()
            torch.cuda.synchronize(dev)
            np.testing.assert_array_equal(mean_out.cpu().numpy().view(np.uint32), want["mean"].view(np.uint32), err_msg=f"replay {r}")
            np.testing.assert_array_equal(logp_out.cpu().numpy().view(np.uint32), want["logp"].view(np.uint32), err_msg=f"replay {r}")
    finally:
        eng.set_stream(None)                                     # the engine is shared: back to its own stream


def test_zero_steps_are_a_no_op(m):
    import torch
    cfg = "two"
    eng = engine(m, cfg)
    dev = torch.device("cuda", eng.device)
    n, d = CONFIGS[cfg][1], dof_of(cfg)
    res = eng.policy_eval(dev_layers(eng, host_layers(cfg)), torch.empty((0, n_inputs(cfg), n), device=dev),
                          actions=torch.empty((0, d, n), device=dev), sigma=1.0, **shape_kw(cfg))
    assert res["mean"].shape == (0, d, n) and res["logp"].shape == (0, n)
    L = m.lib
    arg = L.MtPolicyEval()
    arg.struct_size = C.sizeof(L.MtPolicyEval)
    arg.n_layers, arg.out_act, arg.out_scale, arg.mean_out = 1, L.ACT_TANH, 180.0, 4096
    assert eng._lib.mt_policy_eval(eng._h, C.byref(arg)) == L.MT_OK


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_host_refuses_what_it_can_see(m):
    import torch
    cfg = "two"
    eng = engine(m, cfg)
    L = m.lib
    dev = torch.device("cuda", eng.device)
    _, n, _, T = CONFIGS[cfg][:4]
    d, n_in = dof_of(cfg), n_inputs(cfg)
    layers = dev_layers(eng, host_layers(cfg))
    big = torch.zeros(T * n_in * n + T * d * n, device=dev)       # obs and the mean in one allocation, side by side
    obs, mean = big[:T * n_in * n].view(T, n_in, n), big[T * n_in * n:].view(T, d, n)
    act = torch.zeros((T, d, n), device=dev)
    logp = torch.zeros((T, n), device=dev)
    with pytest.raises(ValueError, match="logp needs actions"):
        eng.policy_eval(layers, obs, logp=True, **shape_kw(cfg))
    with pytest.raises(ValueError, match="sigma"):
        eng.policy_eval(layers, obs, actions=act, sigma=0.0, **shape_kw(cfg))
    with pytest.raises(ValueError, match="n_out"):
        eng.policy_eval(layers, obs, n_out=9, **shape_kw(cfg))
    arg = L.MtPolicyEval()
    arg.struct_size = C.sizeof(L.MtPolicyEval)
    arg.n_steps, arg.n_layers, arg.hidden_act, arg.out_act = T, 2, L.ACT_RELU, L.ACT_TANH
    arg.width[0] = 32
    for l, (w, b) in enumerate(layers):
        arg.weight[l], arg.bias[l] = w.data_ptr(), b.data_ptr()
    arg.out_scale, arg.flags = 180.0, L.POLICY_SEE_POSE
    arg.sigma[:] = [1.0] * L.MT_MAX_DOF
    arg.obs, arg.action, arg.mean_out, arg.logp_out = obs.data_ptr(), act.data_ptr(), mean.data_ptr(), logp.data_ptr()
    arg.obs_ld = arg.act_ld = arg.mean_ld = arg.logp_ld = n

    def refused(word, **change):
        saved = {k: getattr(arg, k) for k in change}
        for k, v in change.items():
            setattr(arg, k, v)
        rc = eng._lib.mt_policy_eval(eng._h, C.byref(arg))
        msg = eng._lib.mt_last_error(eng._h)
        for k, v in saved.items():
            setattr(arg, k, v)
        assert rc == L.MT_ERR_INVALID_ARG and word in msg, (rc, msg)

    refused(b"needs action", action=None)
    refused(b"both NULL", mean_out=None, logp_out=None)
    refused(b"n_out", n_out=9)
    refused(b"obs_ld", obs_ld=n - 1)
    refused(b"mean_ld", mean_ld=n - 1)
    refused(b"act_ld", act_ld=n - 1)
    refused(b"logp_ld", logp_ld=n - 1)
    refused(b"mean_out overlaps obs", mean_out=obs.data_ptr() + 4 * (T * n_in * n - 1))
    refused(b"logp_out overlaps obs", logp_out=obs.data_ptr())
    refused(b"mean_out overlaps action", mean_out=act.data_ptr())
    refused(b"mean_out overlaps logp_out", logp_out=mean.data_ptr() + 4 * n)
    refused(b"overlaps weight", mean_out=layers[0][0].data_ptr())
    arg.sigma[d - 1] = 0.0
    refused(b"sigma")
    arg.sigma[d - 1] = 1.0
    eng.sync()
    assert not mean.cpu().numpy().any() and not logp.cpu().numpy().any()     # nothing was launched
    assert eng._lib.mt_policy_eval(eng._h, C.byref(arg)) == L.MT_OK
    eng.sync()
    # the drop-in class offers the same call
    env = m.Multienv.__new__(m.Multienv)
    env._engine = eng
    got = env.evaluate_policy(layers, obs, **shape_kw(cfg))["mean"]
    eng.sync()
    np.testing.assert_array_equal(got.cpu().numpy(), mean.cpu().numpy())
