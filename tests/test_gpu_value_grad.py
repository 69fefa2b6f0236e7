"""mt_value_grad (StepEngine.value_grad, Multienv.value_gradient): the critic's regression gradient on mt_policy_grad's
kernels, launched with one output.

Held to tests/ac_ref.py (pg_ref.policy_grad with one-output layers, sigma = 1, a = target):
  * the gradient to fp64 within pg_ref.GRAD_TOL x sum_s |c_s (R_s - V_s) dV_s/dtheta_i| per parameter -- the kernel and the
    bound that constant was measured for -- exactly 0 where that sum is 0;
  * the forward pass to eng.values, bit for bit, through a unit probe;
  * the skip rule, determinism across calls and ld's, the refusals; and mt_policy_grad is left as it was.
Shapes: the families of tests/test_gpu_policy_grad.py::CONFIGS, see test_gpu_policy_eval.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ac_ref
import pg_ref
import policy_ref
import test_gpu_policy_grad as base
from test_gpu_policy_grad import dev_layers, engine, n_inputs, padded, to_dev

pytestmark = pytest.mark.gpu

SEED = 0x7A1E
CONFIGS = {k: base.CONFIGS[k] for k in ("one", "two", "pad", "odd", "w1", "w64", "k32")}
ALL = sorted(CONFIGS)


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def kw_of(cfg, **over):
    """The head of a config: its hidden widths and activation, its output activation (tanh heads at out_scale 5)."""
    _, _, _, _, _, _, hidden, out, see_pose = CONFIGS[cfg]
    kw = dict(hidden=hidden, out=out, out_scale=5.0 if out == "tanh" else 1.0, see_pose=see_pose)
    kw.update(over)
    return kw


@functools.lru_cache(maxsize=None)
def head(cfg):
    return policy_ref.make_weights(SEED + len(cfg), n_inputs(cfg), CONFIGS[cfg][5], 1)


_LOGS = {}


def real_logs(m, cfg):
    """Observations of the config's noisy rollout (test_gpu_policy_grad's), the head's values on them, and gae's returns
    and weights (masked: the logs are made without auto-reset) as targets and coef: numpy arrays, computed once."""
    if cfg not in _LOGS:
        eng = engine(m, cfg)
        log = base.real_logs(m, cfg)
        obs = to_dev(eng, log["observations"])
        values = eng.values(dev_layers(eng, head(cfg)), obs, **kw_of(cfg))
        res = eng.gae(to_dev(eng, log["reward"]), to_dev(eng, log["done"]), values, gamma=0.99, lam=0.95, mask_after_done=True,
                      weights=True)
        eng.sync()
        out = {"observations": log["observations"], "targets": res["returns"].cpu().numpy(), "coef": res["weights"].cpu().numpy(),
               "values": values.cpu().numpy()}
        want = ac_ref.gae(log["reward"], log["done"], out["values"], None, 0.99, 0.95, True)
        np.testing.assert_array_equal(out["targets"], want[1])
        np.testing.assert_array_equal(out["coef"], want[2])
        for v in out.values():
            v.setflags(write=False)
        _LOGS[cfg] = out
    return _LOGS[cfg]


def synthetic(cfg):
    _, n, _, T = CONFIGS[cfg][:4]
    rng = np.random.RandomState(SEED % 1000 + len(cfg))
    obs = (40 * rng.randn(T, n_inputs(cfg), n)).astype(np.float32)
    targets = (3 * rng.randn(T, n)).astype(np.float32)
    coef = rng.randn(T, n).astype(np.float32)
    coef[rng.rand(T, n) < 0.1] = 0
    return {"observations": obs, "targets": targets, "coef": coef}


def run(m, cfg, data, ld=None, fill=np.nan, layers=None, **over):
    eng = engine(m, cfg)
    ld = CONFIGS[cfg][2] if ld is None else ld
    kw = kw_of(cfg, scale=1.0 / CONFIGS[cfg][1])
    kw.update(over)
    res = eng.value_grad(dev_layers(eng, head(cfg)) if layers is None else layers, padded(eng, data["observations"], ld, fill),
                         padded(eng, data["targets"], ld, fill), padded(eng, data["coef"], ld, fill), **kw)
    eng.sync()
    if isinstance(res, tuple):
        return res[0].cpu().numpy(), float(res[1].cpu().numpy()[0])
    return res.cpu().numpy()


def reference(cfg, data, dtype=np.float64, scale=None):
    kw = kw_of(cfg)
    obs = np.moveaxis(data["observations"], 0, -2).reshape(data["observations"].shape[1], -1)
    return ac_ref.value_grad(head(cfg), obs, data["targets"].reshape(-1), data["coef"].reshape(-1), kw["hidden"], kw["out"],
                             kw["out_scale"], scale=1.0 / CONFIGS[cfg][1] if scale is None else scale, dtype=dtype)


# ---- 1. the gradient against fp64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["logs", "synthetic"])
@pytest.mark.parametrize("cfg", ALL)
def test_gradient_against_fp64(m, cfg, source):
    data = real_logs(m, cfg) if source == "logs" else synthetic(cfg)
    grad, loss = run(m, cfg, data, loss=True)
    scale = 1.0 / CONFIGS[cfg][1]
    g64, abs_sum, l64 = reference(cfg, data)
    g32, _, _ = reference(cfg, data, dtype=np.float32)
    assert grad.shape == g64.shape == (engine(m, cfg).value_size(CONFIGS[cfg][5], CONFIGS[cfg][8]),) and np.isfinite(grad).all()
    bound = scale * abs_sum
    live = bound > 0
    ratio = float((np.abs(grad - g64)[live] / bound[live]).max())
    ratio32 = float((np.abs(g32 - g64)[live] / bound[live]).max())
    print(f"value_grad {cfg}/{source}: max |grad - fp64| / abs-sum = {ratio:.3e} (numpy fp32 restatement {ratio32:.3e}); "
          f"loss {loss:.6e} vs {l64:.6e}")
    assert (grad[~live] == 0).all()
    assert live.sum() > 0.5 * live.size
    assert ratio <= pg_ref.GRAD_TOL, (ratio, pg_ref.GRAD_TOL)
    d = dict(data)
    d["coef"] = np.abs(data["coef"])
    assert loss <= 0 or (data["coef"] < 0).any()
    assert abs(loss - l64) <= pg_ref.GRAD_TOL * abs(float(reference(cfg, d, scale=1.0)[2])) * scale


# ---- 2. the forward pass is eng.values', bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["one", "two", "pad", "w64", "k32"])
def test_unit_probe_reads_back_the_value(m, cfg):
    import torch
    eng = engine(m, cfg)
    _, n, _, T = CONFIGS[cfg][:4]
    layers = dev_layers(eng, head(cfg))
    kw = kw_of(cfg, out="identity", out_scale=1.0)
    obs = to_dev(eng, real_logs(m, cfg)["observations"])
    v = eng.values(layers, obs, **kw)
    eng.sync()
    v = v.cpu().numpy()
    assert np.isfinite(v).all() and np.abs(v).max() > 0
    zeros = torch.zeros((T, n), dtype=torch.float32, device=obs.device)
    for t, i in ((0, 0), (T - 1, n - 1), (T // 2, n // 2 + 1)):
        coef = torch.zeros((T, n), dtype=torch.float32, device=obs.device)
        coef[t, i] = 1.0
        grad, loss = eng.value_grad(layers, obs, zeros, coef, loss=True, **kw)
        eng.sync()
        # d/db_L of -1/2 (0 - V)^2 = (0 - V) = -V: the output bias is the last word of the flat vector
        assert grad.cpu().numpy()[-1] == -v[t, i], (t, i)
        assert np.float32(loss.cpu().numpy()[0]) == np.float32(-0.5) * pg_ref.fma32(v[t, i], v[t, i], np.float32(0))


# ---- 3. the skip rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["two", "pad", "odd"])
def test_skipped_samples_contribute_exactly_nothing(m, cfg):
    data = {k: np.array(v) for k, v in synthetic(cfg).items()}
    rng = np.random.RandomState(3)
    T, n = data["coef"].shape
    skip = rng.rand(T, n) < 0.5
    data["coef"][skip] = 0
    clean = {k: np.array(v) for k, v in data.items()}
    clean["observations"][np.broadcast_to(skip[:, None], clean["observations"].shape)] = 0
    clean["targets"][skip] = 0
    poison = np.array([np.nan, np.inf, -np.inf, 4e4], dtype=np.float32)
    data["observations"][np.broadcast_to(skip[:, None], data["observations"].shape)] = np.nan
    data["targets"][skip] = poison[rng.randint(0, 4, size=int(skip.sum()))]
    want, want_loss = run(m, cfg, clean, loss=True)
    got, got_loss = run(m, cfg, data, loss=True)
    assert np.isfinite(got).all() and want.any()
    np.testing.assert_array_equal(got, want)
    assert got_loss == want_loss
    # a target of 40000 alone (coef != 0) takes the sample out as well, NaN observations and all
    bad = {k: np.array(v) for k, v in data.items()}
    bad["coef"][skip] = 1.5
    bad["targets"][skip] = 4e4
    np.testing.assert_array_equal(run(m, cfg, bad), want)
    # coef=None weighs every sample by one
    ones = {k: np.array(v) for k, v in clean.items()}
    ones["coef"][:] = 1
    eng = engine(m, cfg)
    g = eng.value_grad(dev_layers(eng, head(cfg)), to_dev(eng, ones["observations"]), to_dev(eng, ones["targets"]),
                       **kw_of(cfg, scale=1.0 / n))
    eng.sync()
    np.testing.assert_array_equal(g.cpu().numpy(), run(m, cfg, ones))


# ---- 4. determinism, and mt_policy_grad is left alone -------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["pad", "odd", "w64"])
def test_same_arguments_same_bits_whatever_the_ld(m, cfg):
    data = real_logs(m, cfg)
    first = run(m, cfg, data)
    np.testing.assert_array_equal(run(m, cfg, data), first)
    n = CONFIGS[cfg][1]
    np.testing.assert_array_equal(run(m, cfg, data, ld=n, fill=0.0), first)
    np.testing.assert_array_equal(run(m, cfg, data, ld=n + 1000, fill=-np.inf), first)
    eng = engine(m, cfg)
    theta = to_dev(eng, pg_ref.flatten(head(cfg)))               # theta as one flat vector is the same head
    assert [tuple(w.shape) for w, _ in eng.unflatten_value(theta, CONFIGS[cfg][5], CONFIGS[cfg][8])] == [w.shape for w, _ in head(cfg)]
    np.testing.assert_array_equal(run(m, cfg, data, layers=theta, widths=CONFIGS[cfg][5]), first)
    env = m.Multienv.__new__(m.Multienv)                          # the drop-in class offers the same call
    env._engine = eng
    got = env.value_gradient(theta, *[to_dev(eng, data[k]) for k in ("observations", "targets", "coef")], widths=CONFIGS[cfg][5],
                             **kw_of(cfg, scale=1.0 / n))
    eng.sync()
    np.testing.assert_array_equal(got.cpu().numpy(), first)


@pytest.mark.parametrize("cfg", ["two", "pad"])
def test_policy_grad_is_what_it_was_around_a_value_grad_call(m, cfg):
    data = base.real_logs(m, cfg)
    before = base.run(m, cfg, data, loss=True)
    value = run(m, cfg, real_logs(m, cfg), loss=True)
    after = base.run(m, cfg, data, loss=True)
    np.testing.assert_array_equal(after[0], before[0])
    assert after[1] == before[1]
    again = run(m, cfg, real_logs(m, cfg), loss=True)
    np.testing.assert_array_equal(again[0], value[0])
    assert again[1] == value[1]
    eng = engine(m, cfg)
    assert eng._pg_workspace.data_ptr() != eng._vg_workspace.data_ptr()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_host_refuses_a_small_workspace_and_aliasing(m):
    import torch
    cfg = "two"
    eng = engine(m, cfg)
    L = m.lib
    dev = torch.device("cuda", eng.device)
    _, n, _, T = CONFIGS[cfg][:4]
    n_in = n_inputs(cfg)
    layers = dev_layers(eng, head(cfg))
    obs = torch.zeros((T, n_in, n), device=dev)
    target = torch.zeros((T, n), device=dev)
    P = eng.value_size(CONFIGS[cfg][5], True)
    assert P == 32 * n_in + 32 + 32 + 1
    grad = torch.zeros(P, device=dev)
    arg = L.MtValueGrad()
    arg.struct_size = C.sizeof(L.MtValueGrad)
    arg.n_steps, arg.n_layers, arg.hidden_act, arg.out_act = T, 2, L.ACT_RELU, L.ACT_IDENTITY
    arg.width[0] = 32
    for l, (w, b) in enumerate(layers):
        arg.weight[l], arg.bias[l] = w.data_ptr(), b.data_ptr()
    arg.out_scale, arg.scale, arg.flags = 1.0, 1.0, L.POLICY_SEE_POSE
    arg.obs, arg.target = obs.data_ptr(), target.data_ptr()
    arg.obs_ld = arg.target_ld = arg.coef_ld = n
    need = eng._lib.mt_value_grad_workspace(eng._h, 2, arg.width, arg.flags, T)
    assert need >= (P + 1) * 4 and need % ((P + 1) * 4) == 0
    assert need < eng._lib.mt_policy_grad_workspace(eng._h, 2, arg.width, arg.flags, T)
    big = torch.zeros(need // 4 + T * n, device=dev)             # the workspace and coef in one allocation, side by side
    ws, coef = big[:need // 4], big[need // 4:].view(T, n)
    arg.coef = coef.data_ptr()
    arg.grad_out, arg.workspace, arg.workspace_bytes = grad.data_ptr(), ws.data_ptr(), need

    def refused(word, **change):
        saved = {k: getattr(arg, k) for k in change}
        for k, v in change.items():
            setattr(arg, k, v)
        rc = eng._lib.mt_value_grad(eng._h, C.byref(arg))
        msg = eng._lib.mt_last_error(eng._h)
        for k, v in saved.items():
            setattr(arg, k, v)
        assert rc == L.MT_ERR_INVALID_ARG and word in msg, (rc, msg)

    refused(b"workspace_bytes is smaller than mt_value_grad_workspace()", workspace_bytes=need - 4)
    refused(b"workspace", workspace=None)
    refused(b"obs / target / coef is NULL", coef=None)
    refused(b"overlaps obs", grad_out=obs.data_ptr() + 4 * (n_in * n - 1))
    refused(b"grad_out overlaps target", grad_out=target.data_ptr())
    refused(b"workspace overlaps coef", workspace=ws.data_ptr() + 4 * T * n)
    refused(b"overlaps weight", grad_out=layers[1][0].data_ptr())
    refused(b"overlaps workspace", grad_out=ws.data_ptr() + 8)
    refused(b"target_ld", target_ld=n - 1)
    refused(b"out_act", out_act=L.ACT_RELU)
    eng.sync()
    assert not grad.cpu().numpy().any()                          # nothing was launched
    assert eng._lib.mt_value_grad(eng._h, C.byref(arg)) == L.MT_OK
    eng.sync()


def test_see_pose_needs_a_joint_count_the_kernels_can_regroup(m):
    """With one output the gradient kernels read x as triples and at most one single word: D = 5 with the pose appended
    (IN = 3 K + 5) is refused as unsupported, and the same arm without the pose is held to fp64 like any other."""
    import torch
    n, K = 256, 2
    eng = m.StepEngine(n, K, dh_table=np.asarray(m.DH7_TABLE, dtype=np.float64)[:5], radius=60.0, return_ring=4)
    try:
        dev = torch.device("cuda", eng.device)
        rng = np.random.RandomState(5)
        obs = (40 * rng.randn(2, 3 * K, n)).astype(np.float32)
        target, coef = (3 * rng.randn(2, n)).astype(np.float32), rng.randn(2, n).astype(np.float32)
        layers = policy_ref.make_weights(SEED, 3 * K, (8,), 1)
        got = eng.value_grad(dev_layers(eng, layers), to_dev(eng, obs), to_dev(eng, target), to_dev(eng, coef))
        eng.sync()
        g64, abs_sum, _ = ac_ref.value_grad(layers, np.moveaxis(obs, 0, -2).reshape(3 * K, -1), target.reshape(-1), coef.reshape(-1),
                                            "tanh", "identity", 1.0)
        assert (np.abs(got.cpu().numpy() - g64) <= pg_ref.GRAD_TOL * abs_sum).all()
        posed = policy_ref.make_weights(SEED, 3 * K + 5, (8,), 1)
        with pytest.raises(m.ManytorError, match="joints"):
            eng.value_grad(dev_layers(eng, posed), torch.zeros((2, 3 * K + 5, n), device=dev), to_dev(eng, target), to_dev(eng, coef),
                           see_pose=True)
        v = eng.values(dev_layers(eng, posed), torch.zeros((2, 3 * K + 5, n), device=dev), see_pose=True)   # the forward pass has no such limit
        eng.sync()
        assert v.shape == (2, n) and np.isfinite(v.cpu().numpy()).all()
    finally:
        eng.close()
