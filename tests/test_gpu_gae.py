"""mt_gae (StepEngine.gae, Multienv.advantages): advantages, value targets and sample weights from rollout_policy's logs
and a critic's values, held to tests/ac_ref.py's fp32 restatement bit for bit -- no tolerance anywhere -- on synthetic logs
and on a real one, at an n_envs that is no multiple of 64 inside a wider ld (pad columns NaN on the way in, a sentinel on
the way out) and at one that is, for T = 1, 3, 7."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ac_ref
import test_gpu_policy_grad as base
from test_gpu_policy_grad import dev_layers, engine, to_dev

pytestmark = pytest.mark.gpu

SEED = 0x6AE
SHAPES = {"odd": 320, "one": 256}       # config of test_gpu_policy_grad (n = 300 / 256) -> ld
CASES = list(itertools.product((1.0, 0.99), (0.0, 0.95, 1.0), (False, True), (False, True)))   # gamma, lambda, last_value, mask


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def synthetic(n, T):
    rng = np.random.RandomState(SEED % 1000 + T + n)
    reward = rng.randint(-128, 128, size=(T, n)).astype(np.int8)
    done = (rng.rand(T, n) < 0.2).astype(np.uint8)
    done[:, :8] = 0                                              # never
    done[0, 8:16] = 1                                            # at t = 0
    return reward, done


_REAL = {}


def real(m, cfg, T):
    """reward / done of a noisy 7-step rollout of the config's policy WITHOUT auto-reset (envs step on behind their done):
    its first T rows."""
    if cfg not in _REAL:
        eng = engine(m, cfg)
        eng.reset_random(SEED, 0)
        kw = base.kw_of(cfg)
        res = eng.rollout_policy(dev_layers(eng, base.host_layers(cfg)), 7, sigma=60.0, seed=SEED, log=True, dry_run=True, **kw)
        eng.sync()
        _REAL[cfg] = res["reward"].cpu().numpy(), res["done"].cpu().numpy()
    return _REAL[cfg][0][:T], _REAL[cfg][1][:T]


def critic(n, T):
    rng = np.random.RandomState(SEED % 1000 + 7 * T + n)
    return (3 * rng.randn(T, n)).astype(np.float32), (3 * rng.randn(n)).astype(np.float32)


def raw_gae(m, eng, reward, done, value, last, gamma, lam, mask, ld, want_ret=True, want_weight=True):
    """mt_gae through the C ABI on (T, ld) buffers: inputs with poison in the pad columns (99 / 1 / NaN), outputs filled with
    a sentinel.  -> the three (T, ld) output buffers as numpy arrays (None where not asked for)."""
    import torch
    L = m.lib
    dev = torch.device("cuda", eng.device)
    T, n = reward.shape
    rbuf = torch.full((T, ld), 99, dtype=torch.int8, device=dev)
    dbuf = torch.full((T, ld), 1, dtype=torch.uint8, device=dev)
    vbuf = torch.full((T, ld + 1), float("nan"), dtype=torch.float32, device=dev)
    rbuf[:, :n], dbuf[:, :n], vbuf[:, :n] = to_dev(eng, reward), to_dev(eng, done), to_dev(eng, value)
    outs = [torch.full((T, ld + q), -5.0, dtype=torch.float32, device=dev) for q in (0, 2, 3)]
    last_d = to_dev(eng, last) if last is not None else None
    arg = L.MtGae()
    arg.struct_size = C.sizeof(L.MtGae)
    arg.n_steps = T
    arg.reward_log, arg.done_log, arg.log_ld = rbuf.data_ptr(), dbuf.data_ptr(), ld
    arg.value, arg.value_ld = vbuf.data_ptr(), ld + 1
    arg.last_value = last_d.data_ptr() if last is not None else None
    arg.gamma, arg.lambda_ = gamma, lam
    arg.adv_out, arg.adv_ld = outs[0].data_ptr(), ld
    if want_ret:
        arg.ret_out, arg.ret_ld = outs[1].data_ptr(), ld + 2
    if want_weight:
        arg.weight_out, arg.weight_ld = outs[2].data_ptr(), ld + 3
    arg.flags = L.GAE_MASK_AFTER_DONE if mask else 0
    assert eng._lib.mt_gae(eng._h, C.byref(arg)) == L.MT_OK, eng._lib.mt_last_error(eng._h)
    eng.sync()
    return [o.cpu().numpy() for o in outs]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("T", [1, 3, 7])
@pytest.mark.parametrize("cfg", sorted(SHAPES))
@pytest.mark.parametrize("source", ["synthetic", "real"])
def test_gae_bit_for_bit(m, cfg, T, source):
    eng = engine(m, cfg)
    n, ld = base.CONFIGS[cfg][1], SHAPES[cfg]
    reward, done = synthetic(n, T) if source == "synthetic" else real(m, cfg, T)
    if source == "real" and T == 7:
        assert done.any() or (reward != 0).any()                 # the log is a log
    value, last = critic(n, T)
    for gamma, lam, with_last, mask in CASES:
        poisoned = np.array(value)
        if mask:                                                 # a masked step's value is never read
            poisoned[1:][np.cumsum(done != 0, axis=0)[:-1] > 0] = np.nan
        got = raw_gae(m, eng, reward, done, poisoned, last if with_last else None, gamma, lam, mask, ld)
        want = ac_ref.gae(reward, done, value, last if with_last else None, gamma, lam, mask)
        for name, g, w in zip(("adv", "ret", "weight"), got, want):
            np.testing.assert_array_equal(bits(g[:, :n]), bits(w), err_msg=f"{name} at gamma {gamma} lambda {lam} last {with_last} mask {mask}")
            assert (g[:, n:] == -5.0).all(), name                # pad columns are not written
        assert np.isfinite(got[0][:, :n]).all()                  # ... nor read: the NaN stayed outside
        if lam == 1.0 and not with_last:                         # no critic: the reward-to-go
            zeros = raw_gae(m, eng, reward, done, np.zeros_like(value), None, gamma, 1.0, mask, ld, want_ret=False, want_weight=False)
            rtg = eng.reward_to_go(to_dev(eng, reward), to_dev(eng, done), gamma, 0.0, mask_after_done=mask)
            eng.sync()
            np.testing.assert_array_equal(bits(zeros[0][:, :n]), bits(rtg.cpu().numpy()))
            assert (zeros[1] == -5.0).all() and (zeros[2] == -5.0).all()     # outputs not asked for are not written


def test_front_end_and_graph_replay(m):
    import torch
    cfg = "odd"
    eng = engine(m, cfg)
    n, T = base.CONFIGS[cfg][1], 7
    dev = torch.device("cuda", eng.device)
    reward, done = real(m, cfg, T)
    value, last = critic(n, T)
    want = ac_ref.gae(reward, done, value, last, 0.99, 0.95, True)
    args = [to_dev(eng, a) for a in (reward, done, value)]
    last_d = to_dev(eng, last)
    res = eng.gae(*args, last_value=last_d, mask_after_done=True, weights=True)
    eng.sync()
    for k, w in zip(("advantages", "returns", "weights"), want):
        np.testing.assert_array_equal(bits(res[k].cpu().numpy()), bits(w), err_msg=k)
    assert sorted(eng.gae(*args, returns=False)) == ["advantages"]
    env = m.Multienv.__new__(m.Multienv)                          # the drop-in class offers the same call
    env._engine = eng
    again = env.advantages(*args, last_value=last_d, mask_after_done=True)
    eng.sync()
    np.testing.assert_array_equal(bits(again["advantages"].cpu().numpy()), bits(want[0]))
    # captured on a side stream, replayed twice
    L = m.lib
    outs = [torch.zeros((T, n), device=dev) for _ in range(3)]
    arg = L.MtGae()
    arg.struct_size = C.sizeof(L.MtGae)
    arg.n_steps = T
    arg.reward_log, arg.done_log, arg.log_ld = args[0].data_ptr(), args[1].data_ptr(), n
    arg.value, arg.value_ld, arg.last_value = args[2].data_ptr(), n, last_d.data_ptr()
    arg.gamma, arg.lambda_, arg.flags = 0.99, 0.95, L.GAE_MASK_AFTER_DONE
    arg.adv_out, arg.ret_out, arg.weight_out = (o.data_ptr() for o in outs)
    arg.adv_ld = arg.ret_ld = arg.weight_ld = n
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    try:
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                assert eng._lib.mt_gae(eng._h, C.byref(arg)) == L.MT_OK
        torch.cuda.synchronize(dev)
        assert not outs[0].cpu().numpy().any()                   # captured, not run
        for r in range(2):
            for o in outs:
                o.fill_(3.0)
            graph.replay()
            torch.cuda.synchronize(dev)
            for o, w in zip(outs, want):
                np.testing.assert_array_equal(bits(o.cpu().numpy()), bits(w), err_msg=f"replay {r}")
    finally:
        eng.set_stream(None)                                     # the engine is shared: back to its own stream


def test_host_refuses_what_it_can_see(m):
    import torch
    cfg = "one"
    eng = engine(m, cfg)
    L = m.lib
    dev = torch.device("cuda", eng.device)
    n, T = base.CONFIGS[cfg][1], 3
    reward = torch.zeros((T, n), dtype=torch.int8, device=dev)
    done = torch.zeros((T, n), dtype=torch.uint8, device=dev)
    big = torch.zeros((5 * T + 1, n), device=dev)                 # value | adv | ret | weight | spare, and last_value
    value, adv, ret, weight, last = big[:T], big[T:2 * T], big[2 * T:3 * T], big[3 * T:4 * T], big[5 * T]
    for kw in (dict(gamma=1.5), dict(gamma=-0.1), dict(lam=1.01), dict(lam=float("nan"))):
        with pytest.raises(ValueError, match="gamma and lam"):
            eng.gae(reward, done, value, **kw)
    with pytest.raises(ValueError):
        eng.gae(reward, done, value[:2])
    arg = L.MtGae()
    arg.struct_size = C.sizeof(L.MtGae)
    arg.n_steps = T
    arg.reward_log, arg.done_log, arg.log_ld = reward.data_ptr(), done.data_ptr(), n
    arg.value, arg.value_ld, arg.last_value = value.data_ptr(), n, last.data_ptr()
    arg.gamma, arg.lambda_ = 0.99, 0.95
    arg.adv_out, arg.ret_out, arg.weight_out = adv.data_ptr(), ret.data_ptr(), weight.data_ptr()
    arg.adv_ld = arg.ret_ld = arg.weight_ld = n

    def refused(word, **change):
        saved = {k: getattr(arg, k) for k in change}
        for k, v in change.items():
            setattr(arg, k, v)
        rc = eng._lib.mt_gae(eng._h, C.byref(arg))
        msg = eng._lib.mt_last_error(eng._h)
        for k, v in saved.items():
            setattr(arg, k, v)
        assert rc == L.MT_ERR_INVALID_ARG and word in msg, (rc, msg)

    refused(b"gamma", gamma=1.0000001)
    refused(b"lambda", lambda_=-1e-9)
    refused(b"adv_out is NULL", adv_out=None)
    refused(b"value is NULL", value=None)
    for name in ("log_ld", "value_ld", "adv_ld", "ret_ld", "weight_ld"):
        refused(name.encode(), **{name: n - 1})
    refused(b"adv_out overlaps value", adv_out=value.data_ptr() + 4 * (T * n - 1))
    refused(b"adv_out overlaps ret_out", adv_out=ret.data_ptr() - 4)
    refused(b"ret_out overlaps weight_out", ret_out=weight.data_ptr() + 4)
    refused(b"weight_out overlaps last_value", weight_out=last.data_ptr() - 4 * (T * n - 1))
    refused(b"ret_out overlaps reward_log", ret_out=reward.data_ptr())
    refused(b"adv_out overlaps done_log", adv_out=done.data_ptr())
    eng.sync()
    big[:T] = 1.0
    assert eng._lib.mt_gae(eng._h, C.byref(arg)) == L.MT_OK
    eng.sync()
    assert (weight.cpu().numpy() == 1).all() and (big[4 * T:5 * T].cpu().numpy() == 0).all()
    arg.n_steps, arg.adv_out = 0, None                           # no step: a no-op
    assert eng._lib.mt_gae(eng._h, C.byref(arg)) == L.MT_OK
