"""mt_ppo_grad (StepEngine.policy_grad(..., old_logp=), Multienv.policy_gradient): PPO's clipped surrogate gradient in one
pass over rollout_policy's logs.

Held to tests/ppo_ref.py:
  * ratio_out to the fp64 exp of the kernel's own fp32 log-ratio x (rebuilt bit for bit from policy_eval's logp), within
    RATIO_TOL (1 + |x|) relative;
  * coef_out and the two counts to the fp32 function of (ratio_out, adv, weight, lo, hi), bit for bit and exactly;
  * grad to mt_policy_grad(coef = coef_out) on the same handle, bit for bit; with old_logp = the current logp, ratio exactly 1
    and grad = mt_policy_grad(coef = fl(weight * adv));
  * grad, loss, kl and sigma_grad to the fp64 restatement within (GRAD_TOL + RATIO_TOL (1 + max |x|)) x their absolute sums;
  * the clamp of x, clip = 0, the shift; the skip rule, the ld's, determinism (twice, under a HIP graph), n_steps == 0 and
    the refusals that need the handle.
Shapes, weights and logs are tests/test_gpu_policy_grad.py's small ones (its engines and logs are shared): one block, two
partials, NaN pad columns, a ragged tile, D = 7, both register extents, two chunks of x; T is 1 or 3.  The advantages have both
signs and about 10 % zeros; old_logp is policy_eval's logp under weights perturbed just far enough -- chosen on the CPU with
ppo_ref -- that max |x| >= 1 and each of the four classes (A > 0 or A < 0, clipped or not) holds at least 2 % of the samples.
"""
import numpy as np
import pytest

import pg_ref
import ppo_ref
import test_gpu_policy_grad as base

pytestmark = pytest.mark.gpu

CASES = ["k32", "odd", "one", "pad", "two", "w5", "w64"]
WEIGHTED = ("pad", "w5", "odd")        # the cases that pass `weights`
SIGMA = base.SIGMA
CLIP = 0.2
SEED = 0x99F0


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def flat(a):
    """(T, rows, n) -> (rows, T n); (T, n) -> (T n,): the sample order of the restatements."""
    return np.moveaxis(a, 0, -2).reshape(a.shape[1], -1) if a.ndim == 3 else a.reshape(-1)


def eval_logp(m, cfg, layers, obs, act):
    eng = base.engine(m, cfg)
    res = eng.policy_eval(base.dev_layers(eng, layers), base.to_dev(eng, obs), actions=base.to_dev(eng, act), sigma=SIGMA, mean=False,
                          **base.kw_of(cfg))
    eng.sync()
    return res["logp"].cpu().numpy()


def perturbed(layers, eps, seed):
    rng = np.random.RandomState(seed)
    return [((w + np.float32(eps) * np.float32(w.std() + 1e-3) * rng.randn(*w.shape)).astype(np.float32),
             (b + np.float32(eps) * np.float32(0.1) * rng.randn(*b.shape)).astype(np.float32)) for w, b in layers]


_CASE = {}


def case(m, cfg):
    """The inputs of a config, computed once and left unchanged: the real logs, adv, weight, old_logp (the device's logp under
    perturbed weights), the current logp (the device's) and x, the kernel's fp32 log-ratio rebuilt from the two."""
    if cfg in _CASE:
        return _CASE[cfg]
    logs = base.real_logs(m, cfg)
    obs, act = logs["observations"], logs["actions"]
    T, n = logs["coef"].shape
    d = base.dof_of(cfg)
    rng = np.random.RandomState(SEED + len(cfg))
    adv = rng.randn(T, n).astype(np.float32)
    adv[rng.rand(T, n) < 0.1] = 0
    weight = rng.choice(np.array([0.0, 0.5, 1.0, 1.0, 2.0], dtype=np.float32), size=(T, n)) if cfg in WEIGHTED else None
    layers = base.host_layers(cfg)
    sig = np.full(d, SIGMA, dtype=np.float32)
    hidden, out = base.CONFIGS[cfg][6], base.CONFIGS[cfg][7]
    A = ppo_ref.advantage(adv, weight).reshape(-1)
    used = ppo_ref.used_samples(flat(act), adv.reshape(-1), None if weight is None else weight.reshape(-1))
    now = ppo_ref.forward(layers, flat(obs), flat(act), sig, hidden, out, 180.0)[2]
    chosen = None
    for eps in (0.01, 0.02, 0.05, 0.1, 0.2, 0.5, 1.0, 2.0):      # the smallest perturbation that fills every class
        then = ppo_ref.forward(perturbed(layers, eps, SEED), flat(obs), flat(act), sig, hidden, out, 180.0)[2]
        x = np.clip(now - then, -ppo_ref.MAX_LOG_RATIO, ppo_ref.MAX_LOG_RATIO)
        frac = ppo_ref.class_fractions(A, ppo_ref.decide(np.exp(x), A.astype(np.float64), used, CLIP), used)
        if min(frac.values()) >= 0.04 and np.abs(x[used]).max() >= 1.5:
            chosen = eps
            break
    assert chosen is not None, f"{cfg}: no perturbation of the ladder fills the four classes"
    old = eval_logp(m, cfg, perturbed(layers, chosen, SEED), obs, act)
    new = eval_logp(m, cfg, layers, obs, act)
    out = {"observations": obs, "actions": act, "adv": adv, "weight": weight, "old": old, "new": new,
           "x": ppo_ref.log_ratio(new, old), "used": used.reshape(T, n), "A": A.reshape(T, n), "eps": chosen}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASE[cfg] = out
    return out


def run(m, cfg, data, ld=None, fill=np.nan, clip=CLIP, plain=False, **over):
    """The call on a config's data (numpy in, numpy out), every array in a buffer of pitch ld whose pad columns hold `fill`."""
    import torch
    eng = base.engine(m, cfg)
    n = base.CONFIGS[cfg][1]
    ld = base.CONFIGS[cfg][2] if ld is None else ld
    pad = lambda a: base.padded(eng, a, ld, fill)
    kw = base.kw_of(cfg, sigma=SIGMA, scale=1.0 / n)
    kw.update(over)
    layers = base.dev_layers(eng, base.host_layers(cfg))
    if plain:                                                    # mt_policy_grad with coef = data["coef"]
        g = eng.policy_grad(layers, pad(data["observations"]), pad(data["actions"]), pad(data["coef"]), **kw)
        eng.sync()
        return g.cpu().numpy()
    T = data["adv"].shape[0]
    bufs = {k: torch.full((T, ld), float(fill), dtype=torch.float32, device=torch.device("cuda", eng.device)) for k in ("ratio", "coef")}
    res = eng.policy_grad(layers, pad(data["observations"]), pad(data["actions"]), pad(data["adv"]), old_logp=pad(data["old"]),
                          weights=None if data.get("weight") is None else pad(data["weight"]), clip=clip,
                          ratio=bufs["ratio"][:, :n], coef_out=bufs["coef"][:, :n], sigma_grad=True, **kw)
    eng.sync()
    out = {k: v.cpu().numpy() for k, v in res.items()}
    for k, b in bufs.items():                                    # the pad columns are as they were
        tail = b[:, n:].cpu().numpy()
        assert (np.isnan(tail).all() if np.isnan(fill) else (tail == fill).all()), f"{k}: a pad column was written"
    out["loss"], out["kl"] = float(out["loss"][0]), float(out["kl"][0])
    out["used"], out["clipped"] = int(out["used"]), int(out["clipped"])
    return out


_RUNS = {}


def default_run(m, cfg):
    if cfg not in _RUNS:
        _RUNS[cfg] = run(m, cfg, case(m, cfg))
    return _RUNS[cfg]


def test_every_case_fills_the_four_classes(m):
    for cfg in CASES:
        c = case(m, cfg)
        used = c["used"]
        ratio = np.exp(c["x"].astype(np.float64)).astype(np.float32)
        frac = ppo_ref.class_fractions(c["A"], ppo_ref.decide(ratio, c["A"], used, CLIP), used)
        zeros = float((c["adv"] == 0).mean())
        print(f"ppo_grad {cfg}: eps {c['eps']}, max |x| {np.abs(c['x'][used]).max():.3f}, zeros {zeros:.3f}, classes {frac}")
        assert min(frac.values()) >= 0.02, (cfg, frac)
        assert np.abs(c["x"][used]).max() >= 1.0
        assert (c["A"][used] > 0).any() and (c["A"][used] < 0).any() and 0.05 < zeros < 0.15


# ---- 1. the ratio -------------------------------------------------------------------------------------------------------
def ratio_error(ratio, x, used):
    want = np.exp(x.astype(np.float64))
    return float((np.abs(ratio.astype(np.float64) - want) / want / (1 + np.abs(x.astype(np.float64))))[used].max())


@pytest.mark.parametrize("cfg", CASES)
def test_ratio_against_fp64_exp(m, cfg):
    c, got = case(m, cfg), default_run(m, cfg)
    used = c["used"]
    err = ratio_error(got["ratio"], c["x"], used)
    print(f"ppo_grad {cfg}: max |ratio - exp(x)| / exp(x) / (1 + |x|) = {err:.3e} over {int(used.sum())} samples (gate {ppo_ref.RATIO_TOL:.3e})")
    assert not got["ratio"][~used].any() and not got["coef"][~used].any()
    assert np.isfinite(got["ratio"]).all()
    assert err <= ppo_ref.RATIO_TOL


# ---- 2. the coefficient and the counts: the fp32 function of the kernel's own ratio --------------------------------------
@pytest.mark.parametrize("cfg", CASES)
def test_coef_and_counts_are_the_fp32_function_of_the_kernels_ratio(m, cfg):
    c, got = case(m, cfg), default_run(m, cfg)
    want, used, clipped = ppo_ref.coef32(got["ratio"], c["adv"], c["weight"], c["used"], CLIP)
    np.testing.assert_array_equal(got["coef"], want)
    assert (got["used"], got["clipped"]) == (used, clipped)
    assert 0 < clipped < used


# ---- 3. the gradient is mt_policy_grad's for that coefficient ------------------------------------------------------------
@pytest.mark.parametrize("cfg", CASES)
def test_grad_is_policy_grads_for_the_same_coef_bit_for_bit(m, cfg):
    c, got = case(m, cfg), default_run(m, cfg)
    plain = run(m, cfg, {"observations": c["observations"], "actions": c["actions"], "coef": got["coef"]}, plain=True)
    assert got["grad"].any()
    np.testing.assert_array_equal(got["grad"], plain)


# ---- 4. the current logp as the old one ----------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [0.2, 0.0, 0.001])
@pytest.mark.parametrize("cfg", ["pad", "two", "w5"])
def test_current_logp_gives_ratio_exactly_one(m, cfg, clip):
    c = dict(case(m, cfg))
    c["old"] = c["new"]
    got = run(m, cfg, c, clip=clip)
    used = c["used"]
    assert (got["ratio"][used] == 1).all() and not got["ratio"][~used].any()
    assert got["clipped"] == 0 and got["used"] == int(used.sum()) and got["kl"] == 0
    np.testing.assert_array_equal(got["coef"], np.where(used, c["A"], np.float32(0)))
    plain = run(m, cfg, {"observations": c["observations"], "actions": c["actions"], "coef": c["A"]}, plain=True)
    np.testing.assert_array_equal(got["grad"], plain)


# ---- 5. the sums against fp64 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CASES)
def test_sums_against_fp64(m, cfg):
    c, got = case(m, cfg), default_run(m, cfg)
    n, d = base.CONFIGS[cfg][1], base.dof_of(cfg)
    scale = 1.0 / n
    w = None if c["weight"] is None else c["weight"].reshape(-1)
    ref = ppo_ref.ppo_grad(base.host_layers(cfg), flat(c["observations"]), flat(c["actions"]), c["adv"].reshape(-1), c["old"].reshape(-1),
                           np.full(d, SIGMA, dtype=np.float32), base.CONFIGS[cfg][6], base.CONFIGS[cfg][7], 180.0, CLIP, weight=w,
                           scale=scale, log_ratio_in=c["x"].reshape(-1), decide_ratio=got["ratio"].reshape(-1))
    assert (ref["used"], ref["clipped"]) == (got["used"], got["clipped"])
    tol = pg_ref.GRAD_TOL + ppo_ref.RATIO_TOL * (1 + float(np.abs(c["x"][c["used"]]).max()))
    bound = scale * ref["grad_abs"]
    live = bound > 0
    figures = {"grad": float((np.abs(got["grad"] - ref["grad"])[live] / bound[live]).max()),
               "loss": abs(got["loss"] - ref["loss"]) / (scale * ref["loss_abs"]),
               "kl": abs(got["kl"] - ref["kl"]) / (scale * ref["kl_abs"]),
               "sigma_grad": float((np.abs(got["sigma_grad"] - ref["sigma_grad"]) / (scale * ref["sigma_abs"])).max())}
    print(f"ppo_grad {cfg}: error / absolute sum {', '.join(f'{k} {v:.3e}' for k, v in figures.items())} (gate {tol:.3e}); "
          f"loss {got['loss']:.6e} vs {ref['loss']:.6e}, kl {got['kl']:.6e} vs {ref['kl']:.6e}")
    assert got["grad"].shape == ref["grad"].shape and np.isfinite(got["grad"]).all()
    assert (got["grad"][~live] == 0).all() and live.sum() > 0.5 * live.size
    assert got["sigma_grad"].shape == (d,) and (ref["sigma_abs"] > 0).all() and ref["loss_abs"] > 0 and ref["kl_abs"] > 0
    for k, v in figures.items():
        assert v <= tol, (k, v, tol)
    assert got["kl"] >= 0


# ---- 6. the clamp, clip = 0, the shift -----------------------------------------------------------------------------------
def test_clamp_no_clipping_and_shift(m):
    cfg = "two"
    c = dict(case(m, cfg))
    rng = np.random.RandomState(8)
    push = rng.choice(np.array([-30.0, 0.0, 30.0], dtype=np.float32), size=c["new"].shape)
    c["old"] = (c["new"] - push).astype(np.float32)              # x = +-30 before the clamp on two thirds of the samples
    x = ppo_ref.log_ratio(c["new"], c["old"])
    used = c["used"]
    assert (x[used] == 20).any() and (x[used] == -20).any() and np.abs(x).max() == 20
    got = run(m, cfg, c)
    assert all(np.isfinite(got[k]).all() for k in ("ratio", "coef", "grad", "sigma_grad")) and np.isfinite([got["loss"], got["kl"]]).all()
    assert ratio_error(got["ratio"], x, used) <= ppo_ref.RATIO_TOL
    assert got["ratio"][used].max() <= np.exp(20.0) * (1 + 21 * ppo_ref.RATIO_TOL) and got["ratio"][used].min() >= np.exp(-20.0) * (1 - 21 * ppo_ref.RATIO_TOL)
    want, n_used, n_clipped = ppo_ref.coef32(got["ratio"], c["adv"], c["weight"], used, CLIP)
    np.testing.assert_array_equal(got["coef"], want)
    assert (got["used"], got["clipped"]) == (n_used, n_clipped)
    # clip = 0 never clips: the importance-weighted policy gradient
    free = run(m, cfg, c, clip=0.0)
    assert free["clipped"] == 0 and free["used"] == n_used
    np.testing.assert_array_equal(free["ratio"], got["ratio"])
    np.testing.assert_array_equal(free["coef"], np.where(used, (got["ratio"] * c["A"]).astype(np.float32), np.float32(0)))
    # a shift is the same as the shift folded into old_logp, up to the roundings of the two ways to x
    c = dict(case(m, cfg))
    d = base.dof_of(cfg)
    sigma_old = np.float32(SIGMA * 1.1)
    shift = np.float32(d * np.log(float(sigma_old) / float(np.float32(SIGMA))))
    assert abs(shift) > 0.3
    shifted = run(m, cfg, c, sigma_old=float(sigma_old))
    np.testing.assert_array_equal(run(m, cfg, c, sigma_old=[float(sigma_old)] * d)["ratio"], shifted["ratio"])
    xs = ppo_ref.log_ratio(c["new"], c["old"], shift)
    assert ratio_error(shifted["ratio"], xs, used) <= ppo_ref.RATIO_TOL        # two fp32 adds, in that order
    folded = dict(c)
    folded["old"] = (c["old"] - shift).astype(np.float32)
    f = run(m, cfg, folded)
    eps = 2.0 ** -24
    slack = eps * (np.abs(c["new"]) + 2 * np.abs(c["old"]) + 2 * abs(float(shift)) + np.abs(xs)) + 2 * ppo_ref.RATIO_TOL * (1 + np.abs(xs))
    rel = np.abs(f["ratio"].astype(np.float64) - shifted["ratio"]) / np.maximum(shifted["ratio"], 1e-30)
    assert (rel[used] <= slack[used] * 1.01).all()
    assert not np.array_equal(shifted["ratio"], default_run(m, cfg)["ratio"])


# ---- 7. the skip rule, the pad columns, the ld's -------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["pad", "odd", "two"])
def test_skipped_samples_contribute_exactly_nothing(m, cfg):
    c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in case(m, cfg).items()}
    rng = np.random.RandomState(3)
    T, n = c["adv"].shape
    if c["weight"] is None:
        c["weight"] = np.ones((T, n), dtype=np.float32)
    pick = rng.randint(0, 4, size=(T, n))                        # 0: stays; 1: adv = 0; 2: weight = 0; 3: an unusable action
    c["adv"][pick == 1] = 0
    c["weight"][pick == 2] = 0
    clean = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    skip = (pick != 0) | (c["adv"] == 0) | (c["weight"] == 0)
    clean["adv"][pick == 3] = 0                                  # the clean twin drops those through adv
    for name in ("observations", "actions"):
        clean[name][np.broadcast_to(skip[:, None], clean[name].shape)] = 0
    clean["old"][skip] = 0
    poison = np.array([np.nan, np.inf, -np.inf, 4e4], dtype=np.float32)
    for name in ("observations", "actions"):
        a = c[name]
        mask = np.broadcast_to(skip[:, None], a.shape)
        a[mask] = poison[rng.randint(0, 4, size=int(mask.sum()))]
    c["actions"][:, 1][pick == 3] = 7                            # one unusable a_j is enough: the others may be anything
    c["actions"][:, 0][pick == 3] = poison[rng.randint(0, 4, size=int((pick == 3).sum()))]
    c["old"][skip] = np.nan
    want, got = run(m, cfg, clean), run(m, cfg, c)
    assert want["used"] == int((~skip).sum()) > 0 and want["clipped"] > 0
    for k in want:
        assert np.isfinite(got[k]).all(), k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    # nothing counts: nothing comes out
    c["adv"][:] = 0
    none = run(m, cfg, c)
    assert not any(np.any(none[k]) for k in none)


@pytest.mark.parametrize("cfg", ["pad", "odd", "w64"])
def test_same_arguments_same_bits_whatever_the_ld(m, cfg):
    c, first = case(m, cfg), default_run(m, cfg)
    n = base.CONFIGS[cfg][1]
    for again in (run(m, cfg, c), run(m, cfg, c, ld=n, fill=0.0), run(m, cfg, c, ld=n + 1000, fill=-np.inf)):
        for k in first:
            np.testing.assert_array_equal(again[k], first[k], err_msg=k)
    # theta as one flat vector is the same policy; the optional outputs are optional
    eng = base.engine(m, cfg)
    theta = base.to_dev(eng, pg_ref.flatten(base.host_layers(cfg)))
    res = eng.policy_grad(theta, *[base.to_dev(eng, c[k]) for k in ("observations", "actions", "adv")], old_logp=base.to_dev(eng, c["old"]),
                          weights=None if c["weight"] is None else base.to_dev(eng, c["weight"]), clip=CLIP, widths=base.CONFIGS[cfg][5],
                          **base.kw_of(cfg, sigma=SIGMA, scale=1.0 / n))
    eng.sync()
    assert sorted(res) == ["clipped", "grad", "kl", "loss", "used"]
    np.testing.assert_array_equal(res["grad"].cpu().numpy(), first["grad"])
    assert (float(res["loss"].cpu()[0]), float(res["kl"].cpu()[0]), int(res["used"]), int(res["clipped"])) == (
        first["loss"], first["kl"], first["used"], first["clipped"])
    # the drop-in class passes the keywords through
    env = m.Multienv.__new__(m.Multienv)
    env._engine = eng
    res = env.policy_gradient(theta, *[base.to_dev(eng, c[k]) for k in ("observations", "actions", "adv")], old_logp=base.to_dev(eng, c["old"]),
                              weights=None if c["weight"] is None else base.to_dev(eng, c["weight"]), clip=CLIP, widths=base.CONFIGS[cfg][5],
                              **base.kw_of(cfg, sigma=SIGMA, scale=1.0 / n))
    eng.sync()
    np.testing.assert_array_equal(res["grad"].cpu().numpy(), first["grad"])


# ---- 8. capture, zero steps, refusals ------------------------------------------------------------------------------------
def test_call_is_capturable_in_a_hip_graph(m):
    import torch
    cfg = "pad"
    eng = base.engine(m, cfg)
    c, want = case(m, cfg), default_run(m, cfg)
    dev = torch.device("cuda", eng.device)
    n, ld = base.CONFIGS[cfg][1], base.CONFIGS[cfg][2]
    layers = base.dev_layers(eng, base.host_layers(cfg))
    args = [base.padded(eng, c[k], ld) for k in ("observations", "actions", "adv")]
    old, weight = base.padded(eng, c["old"], ld), base.padded(eng, c["weight"], ld)
    T = c["adv"].shape[0]
    out = torch.zeros(want["grad"].size, dtype=torch.float32, device=dev)
    ratio = torch.zeros((T, n), dtype=torch.float32, device=dev)
    coef = torch.zeros((T, n), dtype=torch.float32, device=dev)
    kw = base.kw_of(cfg, sigma=SIGMA, scale=1.0 / n, grad_out=out, old_logp=old, weights=weight, clip=CLIP, ratio=ratio, coef_out=coef,
                    sigma_grad=True)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    try:
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                res = eng.policy_grad(layers, *args, **kw)
        torch.cuda.synchronize(dev)
        assert not out.cpu().numpy().any() and not ratio.cpu().numpy().any()      # captured, not run
        for r in range(2):
            out.fill_(3.0)
            ratio.fill_(3.0)
            graph.replay()
            torch.cuda.synchronize(dev)
            np.testing.assert_array_equal(out.cpu().numpy(), want["grad"], err_msg=f"replay {r}")
            np.testing.assert_array_equal(ratio.cpu().numpy(), want["ratio"], err_msg=f"replay {r}")
            np.testing.assert_array_equal(coef.cpu().numpy(), want["coef"], err_msg=f"replay {r}")
            np.testing.assert_array_equal(res["sigma_grad"].cpu().numpy(), want["sigma_grad"], err_msg=f"replay {r}")
            assert (float(res["loss"].cpu()[0]), float(res["kl"].cpu()[0]), int(res["used"]), int(res["clipped"])) == (
                want["loss"], want["kl"], want["used"], want["clipped"])
    finally:
        eng.set_stream(None)                                     # the engine is shared: back to its own stream


def raw_arg(m, cfg, T):
    """A valid struct mt_ppo_grad on a config's engine over zeroed inputs, every output given, and what keeps it alive."""
    import ctypes as C
    import torch
    eng = base.engine(m, cfg)
    L = m.lib
    dev = torch.device("cuda", eng.device)
    n, widths = base.CONFIGS[cfg][1], base.CONFIGS[cfg][5]
    d, n_in = base.dof_of(cfg), base.n_inputs(cfg)
    see_pose = base.CONFIGS[cfg][8]
    layers = base.dev_layers(eng, base.host_layers(cfg))
    P = eng.policy_size(widths, see_pose)
    t = {"obs": torch.zeros((T, n_in, n), device=dev), "action": torch.zeros((T, d, n), device=dev), "adv": torch.zeros((T, n), device=dev),
         "old_logp": torch.zeros((T, n), device=dev), "sample_weight": torch.zeros((T, n), device=dev),
         "ratio_out": torch.full((T, n), 7.0, device=dev), "coef_out": torch.full((T, n), 7.0, device=dev),
         "grad_out": torch.full((P,), 7.0, device=dev), "loss_out": torch.full((1,), 7.0, device=dev),
         "kl_out": torch.full((1,), 7.0, device=dev), "sigma_grad_out": torch.full((d,), 7.0, device=dev),
         "count_out": torch.full((2,), 7, dtype=torch.int64, device=dev), "layers": layers}
    arg = L.MtPpoGrad()
    arg.struct_size = C.sizeof(L.MtPpoGrad)
    arg.n_steps, arg.n_layers = T, len(layers)
    arg.hidden_act = eng._ACTIVATIONS[base.CONFIGS[cfg][6]]
    arg.out_act = eng._ACTIVATIONS[base.CONFIGS[cfg][7]]
    for l, (w, b) in enumerate(layers):
        arg.weight[l], arg.bias[l] = w.data_ptr(), b.data_ptr()
        if l < len(widths):
            arg.width[l] = widths[l]
    arg.out_scale, arg.scale, arg.clip, arg.flags = 180.0, 1.0, CLIP, (L.POLICY_SEE_POSE if see_pose else 0)
    arg.sigma[:] = [1.0] * L.MT_MAX_DOF
    for k in ("obs", "action", "adv", "old_logp", "sample_weight", "ratio_out", "coef_out", "grad_out", "loss_out", "kl_out",
              "sigma_grad_out", "count_out"):
        setattr(arg, k, t[k].data_ptr() if t[k].numel() else None)
    arg.obs_ld = arg.act_ld = arg.adv_ld = arg.old_ld = arg.weight_ld = arg.ratio_ld = arg.coef_ld = n
    need = int(eng._lib.mt_ppo_grad_workspace(eng._h, len(layers), arg.width, arg.flags, T))
    t["ws"] = torch.zeros(need // 4 + 4, device=dev)
    arg.workspace, arg.workspace_bytes = (t["ws"].data_ptr() if need else None), need
    return eng, arg, t, need, P


def test_zero_steps_write_zeros_to_every_output(m):
    import ctypes as C
    eng, arg, t, need, _ = raw_arg(m, "two", 0)
    assert need == 0
    assert eng._lib.mt_ppo_grad(eng._h, C.byref(arg)) == m.lib.MT_OK, eng._lib.mt_last_error(eng._h)
    eng.sync()
    for k in ("grad_out", "loss_out", "kl_out", "sigma_grad_out", "count_out"):
        assert not t[k].cpu().numpy().any(), k
    # ... and through the Python call
    import torch
    dev = t["grad_out"].device
    n, d = base.CONFIGS["two"][1], base.dof_of("two")
    res = eng.policy_grad(t["layers"], torch.empty((0, base.n_inputs("two"), n), device=dev), torch.empty((0, d, n), device=dev),
                          torch.empty((0, n), device=dev), old_logp=torch.empty((0, n), device=dev), sigma=1.0, ratio=True,
                          sigma_grad=True, grad_out=t["grad_out"].fill_(5.0), **base.kw_of("two"))
    eng.sync()
    assert res["grad"] is t["grad_out"] and tuple(res["ratio"].shape) == (0, n)
    assert not any(bool(res[k].cpu().numpy().any()) for k in res)


def test_host_refuses_what_needs_the_handle(m):
    import ctypes as C
    cfg = "two"
    T = base.CONFIGS[cfg][3]
    eng, arg, t, need, P = raw_arg(m, cfg, T)
    L = m.lib
    n, d, n_in = base.CONFIGS[cfg][1], base.dof_of(cfg), base.n_inputs(cfg)
    assert need >= (P + 1 + L.PPO_EXTRA_WORDS) * 4 and need % ((P + 1 + L.PPO_EXTRA_WORDS) * 4) == 0
    assert need // (P + 1 + L.PPO_EXTRA_WORDS) == eng._lib.mt_policy_grad_workspace(eng._h, arg.n_layers, arg.width, arg.flags, T) // (P + 1)
    assert eng._lib.mt_ppo_grad_workspace(eng._h, 4, arg.width, arg.flags, T) == 0
    assert eng._lib.mt_ppo_grad_workspace(eng._h, arg.n_layers, arg.width, 1, T) == 0

    def refused(word, **change):
        saved = {k: getattr(arg, k) for k in change}
        for k, v in change.items():
            setattr(arg, k, v)
        rc = eng._lib.mt_ppo_grad(eng._h, C.byref(arg))
        msg = eng._lib.mt_last_error(eng._h)
        for k, v in saved.items():
            setattr(arg, k, v)
        assert rc == L.MT_ERR_INVALID_ARG and word in msg, (rc, msg, word)

    ptr = lambda k, words=0: t[k].data_ptr() + 4 * words
    refused(b"workspace_bytes", workspace_bytes=need - 4)
    refused(b"workspace", workspace=None)
    refused(b"grad_out", grad_out=None)
    refused(b"old_logp", old_logp=None)
    refused(b"adv", adv=None)
    for k in ("obs_ld", "act_ld", "adv_ld", "old_ld", "weight_ld", "ratio_ld", "coef_ld"):
        refused(k.encode(), **{k: n - 1})
    refused(b"count_out", count_out=ptr("count_out", 1))
    # each output against an input, the weights, another output
    refused(b"grad_out overlaps obs", grad_out=ptr("obs", n_in * n - 1))
    refused(b"grad_out overlaps weight", grad_out=t["layers"][1][0].data_ptr())
    # (a moved output starts where the other buffer starts and is no longer than it: it can reach no third one)
    refused(b"ratio_out overlaps adv", ratio_out=ptr("adv"))
    refused(b"ratio_out overlaps coef_out", ratio_out=ptr("coef_out"))
    refused(b"coef_out overlaps old_logp", coef_out=ptr("old_logp"))
    refused(b"coef_out overlaps sample_weight", coef_out=ptr("sample_weight"))
    refused(b"loss_out overlaps action", loss_out=ptr("action", 5))
    refused(b"loss_out overlaps kl_out", loss_out=ptr("kl_out"))
    refused(b"kl_out overlaps count_out", kl_out=ptr("count_out", 3))
    refused(b"grad_out overlaps sigma_grad_out", sigma_grad_out=ptr("grad_out", P - d))
    refused(b"sigma_grad_out overlaps kl_out", kl_out=ptr("sigma_grad_out", d - 1))
    refused(b"sigma_grad_out overlaps obs", sigma_grad_out=ptr("obs", 3))
    refused(b"count_out overlaps workspace", count_out=t["ws"].data_ptr() + 8)
    refused(b"grad_out overlaps workspace", grad_out=t["ws"].data_ptr() + 8)
    refused(b"workspace overlaps", workspace=ptr("obs"))
    arg.sigma[d - 1] = 0.0
    refused(b"sigma")
    arg.sigma[d - 1] = 1.0
    eng.sync()
    for k in ("grad_out", "loss_out", "kl_out", "sigma_grad_out", "ratio_out", "coef_out"):
        assert (t[k].cpu().numpy() == 7).all(), k                # nothing was launched
    assert eng._lib.mt_ppo_grad(eng._h, C.byref(arg)) == L.MT_OK, eng._lib.mt_last_error(eng._h)
    eng.sync()
    for k in ("grad_out", "loss_out", "kl_out", "sigma_grad_out", "ratio_out", "coef_out", "count_out"):
        assert not t[k].cpu().numpy().any(), k                   # adv is all zeros: every sample is skipped
