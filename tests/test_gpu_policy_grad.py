"""mt_policy_grad / mt_reward_to_go (StepEngine.policy_grad, .reward_to_go, Multienv.policy_gradient): the weighted
log-likelihood gradient of the MLP policy from rollout_policy's logs.

Held to tests/pg_ref.py:
  * the gradient to the fp64 restatement within GRAD_TOL x sum_s |c_s dlogp_s/dtheta_i| per parameter (the natural bound of
    an fp32 sum; the constant is measured, see pg_ref.py), exactly 0 where that sum is 0;
  * the forward pass to rollout_policy's own action_log, bit for bit, through a unit probe;
  * the skip rule, determinism (twice, under a HIP graph, across ld's), the bounds of every read and write, bit for bit;
  * the reward-to-go to its fp32 restatement, bit for bit.
Shapes: the smallest that reach each path -- one block, two partials, three with NaN pad columns, an n_envs that is no
multiple of 64; T = 1 and 3; every hidden-width case of the issue, both register extents, and K = 32 for the first layer's
second chunk of inputs; the 4-joint reference arm and the 7-joint table.
"""
import functools

import numpy as np
import pytest

import pg_ref
import policy_ref

pytestmark = pytest.mark.gpu

SEED = 0x9A4D
NOISE = 20.0          # degrees of exploration noise in the logged rollouts
SIGMA = 20.0          # the likelihood's sigma

#          table   n    ld    T  K   widths    hidden  out         see_pose
CONFIGS = {
    "one": ("ref", 256, 256, 1, 7, (), "tanh", "tanh", False),                  # one block, one layer
    "two": ("ref", 512, 512, 3, 7, (32,), "relu", "identity", True),            # two partials per step, a full extent of 32
    "pad": ("ref", 768, 1024, 3, 7, (33, 64), "tanh", "tanh", False),           # NaN pad columns, the extent of 64, a full layer
    "odd": ("ref", 300, 320, 3, 7, (8, 40), "tanh", "identity", True),          # n_envs no multiple of 64: a ragged last tile
    "w1": ("ref", 256, 256, 1, 7, (1,), "tanh", "tanh", False),                 # width 1
    "w5": ("dh7", 256, 264, 3, 7, (5,), "relu", "tanh", True),                  # D = 7, a width inside a block of eight
    "w64": ("dh7", 512, 512, 1, 7, (64, 64), "tanh", "tanh", False),            # both hidden layers full
    "k32": ("ref", 256, 256, 1, 32, (40,), "tanh", "tanh", True),               # IN = 100: the second chunk of x at extent 64
    "k32s": ("ref", 256, 256, 1, 32, (5, 3), "relu", "tanh", False),            # IN = 96: four chunks of x at extent 32
}
ALL = sorted(CONFIGS)


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def dof_of(cfg):
    return 4 if CONFIGS[cfg][0] == "ref" else 7


def n_inputs(cfg):
    return 3 * CONFIGS[cfg][4] + (dof_of(cfg) if CONFIGS[cfg][8] else 0)


_ENGINES = {}


def engine(m, cfg):
    """One engine per (table, n, K), shared by the tests: policy_grad reads nothing resident."""
    table, n, _, _, K = CONFIGS[cfg][:5]
    key = (table, n, K)
    if key not in _ENGINES:
        dh, radius = ((np.asarray(m.REF_DH_TABLE, dtype=np.float64), 51.3) if table == "ref"
                      else (np.asarray(m.DH7_TABLE, dtype=np.float64), 92.6))
        _ENGINES[key] = m.StepEngine(n, K, dh_table=dh, radius=radius, return_ring=4)
    return _ENGINES[key]


@functools.lru_cache(maxsize=None)
def host_layers(cfg):
    return policy_ref.make_weights(SEED + len(cfg), n_inputs(cfg), CONFIGS[cfg][5], dof_of(cfg))


def to_dev(eng, a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", eng.device))


def dev_layers(eng, layers):
    return [(to_dev(eng, w), to_dev(eng, b)) for w, b in layers]


def kw_of(cfg, **over):
    _, _, _, _, _, _, hidden, out, see_pose = CONFIGS[cfg]
    kw = dict(hidden=hidden, out=out, see_pose=see_pose)
    kw.update(over)
    return kw


_LOGS = {}


def real_logs(m, cfg):
    """obs, actions, reward, done of a noisy rollout_policy call on the config's weights, and coef = its reward-to-go
    (restated on the host, gamma 0.99, baseline 0.125): numpy arrays, computed once."""
    if cfg not in _LOGS:
        eng = engine(m, cfg)
        T = CONFIGS[cfg][3]
        eng.reset_random(SEED, 0)
        res = eng.rollout_policy(dev_layers(eng, host_layers(cfg)), T, sigma=NOISE, seed=SEED, log=True, actions=True,
                                 observations=True, dry_run=True, **kw_of(cfg))
        eng.sync()
        out = {k: v.cpu().numpy() for k, v in res.items()}
        out["coef"] = pg_ref.reward_to_go(out["reward"], out["done"], 0.99, 0.125)
        for v in out.values():
            v.setflags(write=False)
        _LOGS[cfg] = out
    return _LOGS[cfg]


def synthetic(cfg):
    """Inputs no rollout made: observations and actions of the logs' magnitude, coef of both signs and a few zeros."""
    _, n, _, T = CONFIGS[cfg][:4]
    rng = np.random.RandomState(SEED % 1000 + len(cfg))
    obs = (40 * rng.randn(T, n_inputs(cfg), n)).astype(np.float32)
    act = (90 * rng.randn(T, dof_of(cfg), n)).astype(np.float32)
    coef = rng.randn(T, n).astype(np.float32)
    coef[rng.rand(T, n) < 0.1] = 0
    return {"observations": obs, "actions": act, "coef": coef}


def padded(eng, a, ld, fill=np.nan):
    """a (..., n) in a (..., ld) device buffer whose pad columns hold `fill`; -> the [..., :n] view the call reads in place."""
    import torch
    n = a.shape[-1]
    buf = torch.full(a.shape[:-1] + (ld,), fill, dtype=torch.float32, device=torch.device("cuda", eng.device))
    buf[..., :n] = to_dev(eng, a)
    return buf[..., :n]


def run(m, cfg, data, ld=None, fill=np.nan, layers=None, **over):
    eng = engine(m, cfg)
    ld = CONFIGS[cfg][2] if ld is None else ld
    kw = kw_of(cfg, sigma=SIGMA, scale=1.0 / CONFIGS[cfg][1])
    kw.update(over)
    res = eng.policy_grad(dev_layers(eng, host_layers(cfg)) if layers is None else layers, padded(eng, data["observations"], ld, fill),
                          padded(eng, data["actions"], ld, fill), padded(eng, data["coef"], ld, fill), **kw)
    eng.sync()
    if isinstance(res, tuple):
        return res[0].cpu().numpy(), float(res[1].cpu().numpy()[0])
    return res.cpu().numpy()


def reference(cfg, data, dtype=np.float64, **over):
    n = CONFIGS[cfg][1]
    flat = lambda a: np.moveaxis(a, 0, -2).reshape(a.shape[1], -1) if a.ndim == 3 else a.reshape(-1)
    kw = dict(sigma=np.full(dof_of(cfg), SIGMA, dtype=np.float32), hidden=CONFIGS[cfg][6], out=CONFIGS[cfg][7], out_scale=180.0,
              scale=1.0 / n)
    kw.update(over)
    return pg_ref.policy_grad(host_layers(cfg), flat(data["observations"]), flat(data["actions"]), flat(data["coef"]),
                              kw["sigma"], kw["hidden"], kw["out"], kw["out_scale"], scale=kw["scale"], dtype=dtype)


# ---- 1. the gradient against fp64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["logs", "synthetic"])
@pytest.mark.parametrize("cfg", ALL)
def test_gradient_against_fp64(m, cfg, source):
    data = real_logs(m, cfg) if source == "logs" else synthetic(cfg)
    grad, loss = run(m, cfg, data, loss=True)
    scale = 1.0 / CONFIGS[cfg][1]
    g64, abs_sum, l64 = reference(cfg, data)
    g32, _, _ = reference(cfg, data, dtype=np.float32)
    assert grad.shape == g64.shape and np.isfinite(grad).all()
    bound = scale * abs_sum
    live = bound > 0
    ratio = float((np.abs(grad - g64)[live] / bound[live]).max())
    ratio32 = float((np.abs(g32 - g64)[live] / bound[live]).max())
    print(f"policy_grad {cfg}/{source}: max |grad - fp64| / abs-sum = {ratio:.3e} (numpy fp32 restatement {ratio32:.3e}); "
          f"loss {loss:.6e} vs {l64:.6e}")
    assert (grad[~live] == 0).all()
    assert live.sum() > 0.5 * live.size
    assert ratio <= pg_ref.GRAD_TOL, (ratio, pg_ref.GRAD_TOL)
    # the loss is one fp32 sum of S terms of one sign per coefficient sign: the same bound, on the sum of |terms|
    keep = pg_ref.usable_samples(np.moveaxis(data["actions"], 0, -2).reshape(dof_of(cfg), -1), data["coef"].reshape(-1))
    assert keep.any()
    assert abs(loss - l64) <= pg_ref.GRAD_TOL * _abs_loss(cfg, data) * scale


def _abs_loss(cfg, data):
    d = dict(data)
    d["coef"] = np.abs(data["coef"])
    return abs(float(reference(cfg, d, scale=1.0)[2]))


# ---- 2. the forward pass is rollout_policy's, bit for bit --------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["one", "two", "pad", "w5", "k32"])
def test_unit_probe_reads_back_rollout_policys_action(m, cfg):
    import torch
    eng = engine(m, cfg)
    _, n, _, T = CONFIGS[cfg][:4]
    d = dof_of(cfg)
    layers = dev_layers(eng, host_layers(cfg))
    kw = kw_of(cfg, out="identity")
    eng.reset_random(SEED, 1)
    res = eng.rollout_policy(layers, T, out_scale=1.0, lo=-30000.0, hi=30000.0, seed=SEED, actions=True, observations=True,
                             dry_run=True, **kw)
    eng.sync()
    mu = res["actions"].cpu().numpy()
    assert np.isfinite(mu).all() and np.abs(mu).max() > 0
    zeros = torch.zeros_like(res["actions"])
    for t, i in ((0, 0), (T - 1, n - 1), (T // 2, n // 2 + 1)):
        coef = torch.zeros((T, n), dtype=torch.float32, device=zeros.device)
        coef[t, i] = 1.0
        grad, loss = eng.policy_grad(layers, res["observations"], zeros, coef, sigma=1.0, out_scale=1.0, loss=True, **kw)
        eng.sync()
        grad = grad.cpu().numpy()
        # d logp / d b_L = (a - mu) / sigma^2 * out_scale = -mu: the output bias is the last D words of the flat vector
        np.testing.assert_array_equal(grad[-d:], -mu[t, :, i], err_msg=f"sample {(t, i)}")
        lp = np.float32(0)
        for j in range(d):                                      # the kernel's chain: lp = fma(e, e, lp), loss = c * (-0.5 lp)
            lp = pg_ref.fma32(mu[t, j, i], mu[t, j, i], lp)
        assert np.float32(loss.cpu().numpy()[0]) == np.float32(-0.5) * lp


# ---- 3. the skip rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["two", "pad", "odd"])
def test_skipped_samples_contribute_exactly_nothing(m, cfg):
    data = {k: np.array(v) for k, v in real_logs(m, cfg).items() if k in ("observations", "actions", "coef")}
    rng = np.random.RandomState(3)
    T, n = data["coef"].shape
    skip = rng.rand(T, n) < 0.5
    data["coef"][skip] = 0
    clean = {k: np.array(v) for k, v in data.items()}
    clean["observations"][np.broadcast_to(skip[:, None], clean["observations"].shape)] = 0
    clean["actions"][np.broadcast_to(skip[:, None], clean["actions"].shape)] = 0
    poison = np.array([np.nan, np.inf, -np.inf, 4e4], dtype=np.float32)
    for name in ("observations", "actions"):
        a = data[name]
        mask = np.broadcast_to(skip[:, None], a.shape)
        a[mask] = poison[rng.randint(0, 4, size=int(mask.sum()))]
    want, want_loss = run(m, cfg, clean, loss=True)
    got, got_loss = run(m, cfg, data, loss=True)
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got, want)
    assert got_loss == want_loss
    # an unusable action alone (coef != 0) takes the sample out as well, NaN observations and all
    bad = {k: np.array(v) for k, v in clean.items()}
    bad["coef"][skip] = 1.5
    bad["actions"][:, 0][skip] = 4e4
    bad["observations"][np.broadcast_to(skip[:, None], bad["observations"].shape)] = np.nan
    np.testing.assert_array_equal(run(m, cfg, bad), want)
    # nothing counts: nothing comes out
    none = {k: np.array(v) for k, v in data.items()}
    none["coef"][:] = 0
    z, zl = run(m, cfg, none, loss=True)
    assert not z.any() and zl == 0


def test_zero_steps_write_zeros(m):
    import torch
    cfg = "two"
    eng = engine(m, cfg)
    n, d = CONFIGS[cfg][1], dof_of(cfg)
    dev = torch.device("cuda", eng.device)
    out = torch.full((eng.policy_size(CONFIGS[cfg][5], True),), 7.0, dtype=torch.float32, device=dev)
    g, loss = eng.policy_grad(dev_layers(eng, host_layers(cfg)), torch.empty((0, n_inputs(cfg), n), device=dev),
                              torch.empty((0, d, n), device=dev), torch.empty((0, n), device=dev), sigma=1.0, grad_out=out, loss=True,
                              **kw_of(cfg))
    eng.sync()
    assert g is out and not out.cpu().numpy().any() and float(loss.cpu()[0]) == 0


# ---- 4. determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["pad", "odd", "w64"])
def test_same_arguments_same_bits_whatever_the_ld(m, cfg):
    data = real_logs(m, cfg)
    first = run(m, cfg, data)
    np.testing.assert_array_equal(run(m, cfg, data), first)
    n = CONFIGS[cfg][1]
    np.testing.assert_array_equal(run(m, cfg, data, ld=n, fill=0.0), first)
    np.testing.assert_array_equal(run(m, cfg, data, ld=n + 1000, fill=-np.inf), first)
    # theta as one flat vector is the same policy
    eng = engine(m, cfg)
    theta = to_dev(eng, pg_ref.flatten(host_layers(cfg)))
    np.testing.assert_array_equal(run(m, cfg, data, layers=theta, widths=CONFIGS[cfg][5]), first)


def test_call_is_capturable_in_a_hip_graph(m):
    import torch
    cfg = "pad"
    eng = engine(m, cfg)
    data = real_logs(m, cfg)
    want = run(m, cfg, data)
    dev = torch.device("cuda", eng.device)
    ld = CONFIGS[cfg][2]
    layers = dev_layers(eng, host_layers(cfg))
    args = [padded(eng, data[k], ld) for k in ("observations", "actions", "coef")]
    out = torch.zeros(want.size, dtype=torch.float32, device=dev)
    kw = kw_of(cfg, sigma=SIGMA, scale=1.0 / CONFIGS[cfg][1], grad_out=out)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    try:
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                eng.policy_grad(layers, *args, **kw)
        torch.cuda.synchronize(dev)
        assert not out.cpu().numpy().any()                       # captured, not run
        for r in range(2):
            out.fill_(3.0)
            graph.replay()
            torch.cuda.synchronize(dev)
            np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"replay {r}")
    finally:
        eng.set_stream(None)                                     # the engine is shared: back to its own stream


# ---- 5. bounds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["w1", "w5", "pad"])
def test_nothing_outside_the_arguments_is_read_or_written(m, cfg):
    import torch
    eng = engine(m, cfg)
    dev = torch.device("cuda", eng.device)
    data = real_logs(m, cfg)
    want = run(m, cfg, data)
    layers = []
    for w, b in host_layers(cfg):                                # every matrix and vector inside NaN, 3 words of it on each side
        pair = []
        for a in (w, b):
            buf = torch.full((a.size + 6,), float("nan"), dtype=torch.float32, device=dev)
            buf[3:3 + a.size] = to_dev(eng, a.reshape(-1))
            pair.append(buf[3:3 + a.size].view(a.shape))
        layers.append(tuple(pair))
    ld = CONFIGS[cfg][2] + 5
    bufs = []
    for k in ("observations", "actions", "coef"):                # a NaN row in front of and behind every log, NaN pad columns
        a = data[k]
        rows = int(np.prod(a.shape[:-1]))
        buf = torch.full((rows + 2, ld), float("nan"), dtype=torch.float32, device=dev)
        view = buf[1:rows + 1].view(a.shape[:-1] + (ld,))[..., :a.shape[-1]]
        view.copy_(to_dev(eng, a))
        bufs.append(view)
    P = want.size
    sentinel = torch.full((P + 64,), -123.25, dtype=torch.float32, device=dev)
    got = eng.policy_grad(layers, *bufs, grad_out=sentinel[32:32 + P], **kw_of(cfg, sigma=SIGMA, scale=1.0 / CONFIGS[cfg][1]))
    eng.sync()
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    s = sentinel.cpu().numpy()
    assert (s[:32] == -123.25).all() and (s[32 + P:] == -123.25).all()
    assert (want != -123.25).all()                               # exactly P words changed


def test_host_refuses_a_small_workspace_and_aliasing(m):
    import ctypes as C
    import torch
    cfg = "two"
    eng = engine(m, cfg)
    L = m.lib
    dev = torch.device("cuda", eng.device)
    _, n, _, T = CONFIGS[cfg][:4]
    d, n_in = dof_of(cfg), n_inputs(cfg)
    layers = dev_layers(eng, host_layers(cfg))
    obs = torch.zeros((T, n_in, n), device=dev)
    act = torch.zeros((T, d, n), device=dev)
    coef = torch.zeros((T, n), device=dev)
    P = eng.policy_size(CONFIGS[cfg][5], True)
    grad = torch.zeros(P, device=dev)
    arg = L.MtPolicyGrad()
    arg.struct_size = C.sizeof(L.MtPolicyGrad)
    arg.n_steps, arg.n_layers, arg.hidden_act, arg.out_act = T, 2, L.ACT_RELU, L.ACT_IDENTITY
    arg.width[0] = 32
    for l, (w, b) in enumerate(layers):
        arg.weight[l], arg.bias[l] = w.data_ptr(), b.data_ptr()
    arg.out_scale, arg.scale, arg.flags = 180.0, 1.0, L.POLICY_SEE_POSE
    arg.sigma[:] = [1.0] * L.MT_MAX_DOF
    arg.obs, arg.action, arg.coef = obs.data_ptr(), act.data_ptr(), coef.data_ptr()
    arg.obs_ld = arg.act_ld = arg.coef_ld = n
    need = eng._lib.mt_policy_grad_workspace(eng._h, 2, arg.width, arg.flags, T)
    assert need >= (P + 1) * 4 and need % ((P + 1) * 4) == 0
    big = torch.zeros(need // 4 + T * n, device=dev)             # the workspace and coef in one allocation, side by side
    ws, coef = big[:need // 4], big[need // 4:].view(T, n)
    arg.coef = coef.data_ptr()
    arg.grad_out, arg.workspace, arg.workspace_bytes = grad.data_ptr(), ws.data_ptr(), need

    def refused(word, **change):
        saved = {k: getattr(arg, k) for k in change}
        for k, v in change.items():
            setattr(arg, k, v)
        rc = eng._lib.mt_policy_grad(eng._h, C.byref(arg))
        msg = eng._lib.mt_last_error(eng._h)
        for k, v in saved.items():
            setattr(arg, k, v)
        assert rc == L.MT_ERR_INVALID_ARG and word in msg, (rc, msg)

    refused(b"workspace_bytes", workspace_bytes=need - 4)
    refused(b"workspace", workspace=None)
    refused(b"overlaps obs", grad_out=obs.data_ptr() + 4 * (n_in * n - 1))
    refused(b"workspace overlaps coef", workspace=ws.data_ptr() + 4 * T * n)
    refused(b"overlaps weight", grad_out=layers[1][0].data_ptr())
    refused(b"overlaps workspace", grad_out=ws.data_ptr() + 8)
    refused(b"obs_ld", obs_ld=n - 1)
    arg.sigma[d - 1] = 0.0
    refused(b"sigma")
    arg.sigma[d - 1] = 1.0
    eng.sync()
    assert not grad.cpu().numpy().any()                          # nothing was launched
    assert eng._lib.mt_policy_grad(eng._h, C.byref(arg)) == L.MT_OK
    eng.sync()


# ---- 6. reward_to_go ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma, baseline", [(1.0, 0.0), (0.5, 0.25), (0.99, -1.7)])
@pytest.mark.parametrize("mask", [False, True])
def test_reward_to_go_bit_for_bit(m, gamma, baseline, mask):
    import torch
    cfg = "odd"
    eng = engine(m, cfg)
    n, T, ld = CONFIGS[cfg][1], 11, 333
    rng = np.random.RandomState(17)
    reward = rng.randint(-1, 2, size=(T, n)).astype(np.int8)
    done = (rng.rand(T, n) < 0.15).astype(np.uint8)
    done[:, :8] = 0                                              # never
    done[0, 8:16] = 1                                            # at t = 0
    done[:, 16:24] = 0
    done[T - 1, 16:24] = 1                                       # at T - 1 only
    dev = torch.device("cuda", eng.device)
    rbuf = torch.full((T, ld), 99, dtype=torch.int8, device=dev)
    dbuf = torch.full((T, ld), 1, dtype=torch.uint8, device=dev)
    rbuf[:, :n], dbuf[:, :n] = to_dev(eng, reward), to_dev(eng, done)
    obuf = torch.full((T, ld + 3), -5.0, dtype=torch.float32, device=dev)
    got = eng.reward_to_go(rbuf[:, :n], dbuf[:, :n], gamma, baseline, mask_after_done=mask, out=obuf[:, :n])
    eng.sync()
    want = pg_ref.reward_to_go(reward, done, gamma, baseline, mask)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert (obuf[:, n:].cpu().numpy() == -5.0).all()
    if gamma == 1.0 and baseline == 0.0:
        np.testing.assert_array_equal(want, np.round(want))
    dense = eng.reward_to_go(to_dev(eng, reward), to_dev(eng, done), gamma, baseline, mask_after_done=mask)
    eng.sync()
    np.testing.assert_array_equal(dense.cpu().numpy(), want)


# ---- 7. closing the loop ------------------------------------------------------------------------------------------------
STATE = ("F_ACTIONS", "F_GOALS", "F_POINTS", "F_ALIVE", "F_TOTAL_REWARD", "F_EPISODES", "F_LAST_RETURN", "F_RETURN_RING", "F_OBS",
         "F_REWARD", "F_DONE", "F_DONE_BITS", "F_EE")


def test_one_reinforce_iteration_closes_the_loop(m):
    cfg = "two"
    eng = engine(m, cfg)
    _, n, _, T, _, widths = CONFIGS[cfg][:6]
    kw = kw_of(cfg)
    theta = to_dev(eng, pg_ref.flatten(host_layers(cfg)))
    eng.reset_random(SEED, 2)
    res = eng.rollout_policy(eng.unflatten_policy(theta, widths, kw["see_pose"]), T, sigma=NOISE, seed=SEED, log=True, actions=True,
                             observations=True, **kw)
    eng.sync()
    before = {f: eng.get(getattr(m.lib, f)) for f in STATE}
    bad0 = eng.bad_action_count()
    coef = eng.reward_to_go(res["reward"], res["done"], 0.99, 0.0, mask_after_done=True)
    grad = eng.policy_grad(theta, res["observations"], res["actions"], coef, sigma=NOISE, widths=widths, scale=1.0 / n, **kw)
    eng.sync()
    after = {f: eng.get(getattr(m.lib, f)) for f in STATE}
    for f in STATE:
        np.testing.assert_array_equal(after[f], before[f], err_msg=f)
    assert eng.bad_action_count() == bad0
    g = grad.cpu().numpy()
    assert g.shape == (eng.policy_size(widths, kw["see_pose"]),) and np.isfinite(g).all()
    want = pg_ref.policy_grad(host_layers(cfg), *[np.moveaxis(res[k].cpu().numpy(), 0, -2).reshape(res[k].shape[1], -1)
                                                  for k in ("observations", "actions")],
                              coef.cpu().numpy().reshape(-1), np.full(dof_of(cfg), NOISE), kw["hidden"], kw["out"], 180.0, scale=1.0 / n)
    live = want[1] > 0
    assert (np.abs(g - want[0])[live] <= pg_ref.GRAD_TOL * want[1][live] / n).all()
    theta2 = theta + 1e-4 * grad
    out = eng.rollout_policy(eng.unflatten_policy(theta2, widths, kw["see_pose"]), T, seed=SEED, returns=True, **kw)
    eng.sync()
    assert np.isfinite(out["returns"].cpu().numpy()).all()
    # the drop-in class offers the same call
    env = m.Multienv.__new__(m.Multienv)
    env._engine = eng
    np.testing.assert_array_equal(env.policy_gradient(theta, res["observations"], res["actions"], coef, sigma=NOISE, widths=widths,
                                                      scale=1.0 / n, **kw).cpu().numpy(), g)
