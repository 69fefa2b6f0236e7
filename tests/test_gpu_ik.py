"""mt_jacobian / mt_ik (StepEngine.jacobian, .ik, Multienv.reach_actions): the position Jacobian of the pickup frame and the
batched damped-least-squares solver, held to tests/ik_ref.py in fp64.

Arms (ik_ref.ARMS): the reference arm and the 7-joint arm through their compile-time tables, the reference arm with
specialize=False, runtime tables of D = 2, 3, 6 and 8, and a 6-joint arm with ee_frame=-2.
Shapes: n = 200 in ld = 256 (one block, no multiple of 64, NaN pad columns), n = 600 (three blocks, ld = n) and n = 4 096
where a share is measured.  K = 7, one K = 32 case.
"""
import ctypes as C

import numpy as np
import pytest

import ik_ref

pytestmark = pytest.mark.gpu

SEED = 0x1C5EED
SHAPES = [(200, 256), (600, 600)]
ALL = sorted(ik_ref.ARMS)


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


_ENGINES = {}


def engine(m, arm, n, K=7, tag=0, **kw):
    key = (arm, n, K, tag, tuple(sorted(kw.items())))
    if key not in _ENGINES:
        table, radius, ee, spec = ik_ref.ARMS[arm]
        opts = dict(dh_table=table, radius=radius, ee_frame=ee, specialize=spec)
        opts.update(kw)
        _ENGINES[key] = m.StepEngine(n, K, **opts)
    return _ENGINES[key]


def to_dev(eng, a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", eng.device))


def rows_in(eng, a, ld):
    """Env-major (n, rows) -> the [..., :n] view of a (rows, ld) device buffer whose pad columns hold NaN."""
    import torch
    n = a.shape[0]
    buf = torch.full((a.shape[1], ld), np.nan, dtype=torch.float32, device=torch.device("cuda", eng.device))
    buf[:, :n] = to_dev(eng, np.ascontiguousarray(a.T.astype(np.float32)))
    return buf[:, :n]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def solve(eng, x=None, q0=None, ld=None, index=None, **kw):
    """ik() writing into [..., :n] views of (.., ld) buffers -> env-major numpy arrays; the pad columns must keep their
    sentinel (NaN, -7 for the integer rows)."""
    import torch
    n, d = eng.n_envs, eng.dof
    ld = n if ld is None else ld
    dev = torch.device("cuda", eng.device)
    ang = torch.full((d, ld), np.nan, dtype=torch.float32, device=dev)
    res = torch.full((ld,), np.nan, dtype=torch.float32, device=dev)
    stp = torch.full((ld,), -7, dtype=torch.int32, device=dev)
    idx = torch.full((ld,), -7, dtype=torch.int32, device=dev)
    nearest = x is None
    out = eng.ik(None if nearest else rows_in(eng, x, ld), None if q0 is None else rows_in(eng, q0, ld), angles=ang[:, :n],
                 residual=res[:n], steps=stp[:n], index=idx[:n] if nearest and index is not False else None, **kw)
    eng.sync()
    assert out["angles"].data_ptr() == ang.data_ptr()
    assert torch.isnan(ang[:, n:]).all() and torch.isnan(res[n:]).all() and (stp[n:] == -7).all() and (idx[n:] == -7).all()
    got = dict(angles=ang[:, :n].cpu().numpy().T.copy(), residual=res[:n].cpu().numpy(), steps=stp[:n].cpu().numpy())
    if nearest and index is not False:
        got["index"] = idx[:n].cpu().numpy()
    return got


# ---- 1. the Jacobian -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, ld", SHAPES)
@pytest.mark.parametrize("arm", ALL)
def test_jacobian_against_fp64(m, arm, n, ld):
    import torch
    eng = engine(m, arm, n)
    table, ee = ik_ref.arm_table(arm), ik_ref.ARMS[arm][2]
    d = eng.dof
    q = ik_ref.pose_case(arm, n)
    buf = torch.full((d, 3, ld), np.nan, dtype=torch.float32, device=torch.device("cuda", eng.device))
    J, p = eng.jacobian(rows_in(eng, q, ld), out=buf[..., :n].permute(1, 0, 2), position=True)
    eng.sync()
    assert tuple(J.shape) == (3, d, n) and J.data_ptr() == buf.data_ptr() and torch.isnan(buf[..., n:]).all()
    got, pos = J.cpu().numpy().transpose(2, 0, 1), p.cpu().numpy().T
    want, wpos = ik_ref.jacobian(q, table, ee)
    ej, ep = float(np.abs(got - want).max()), float(np.abs(pos - wpos).max())
    print(f"jacobian {arm} n={n}: max |J - fp64| = {ej:.3e} per degree, max |p - fp64| = {ep:.3e}")
    f = ik_ref.resolve_frame(ee, d)
    assert (got[:, :, f + 1:] == 0.0).all() and not np.signbit(got[:, :, f + 1:]).any()
    assert np.abs(got).max() > 0.1
    assert ej <= ik_ref.JAC_TOL and ep <= ik_ref.POS_TOL


def test_jacobian_of_the_resident_pose(m):
    eng = engine(m, "ref", 600)
    eng.reset_random(SEED, 0)
    eng.rollout(2, SEED, 0)
    q = eng.goals()
    J = eng.jacobian()
    again = eng.jacobian(rows_in(eng, q, 640))
    eng.sync()
    np.testing.assert_array_equal(bits(J.cpu().numpy()), bits(again.cpu().numpy()))
    assert tuple(J.shape) == (3, 4, 600)


# ---- 2. one iteration ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, ld", SHAPES)
@pytest.mark.parametrize("arm", ALL)
def test_one_iteration_against_fp64(m, arm, n, ld):
    eng = engine(m, arm, n)
    table, ee = ik_ref.arm_table(arm), ik_ref.ARMS[arm][2]
    x, q0 = ik_ref.step_case(arm, n)
    got = solve(eng, x, q0, ld, iters=1, tol=0.0, wrap=False)
    want, _, _ = ik_ref.ik(x, q0, table, ee, iters=1)
    err = float(np.abs(got["angles"] - want).max())
    back = ik_ref.box(x.astype(np.float64) - ik_ref.position(got["angles"], table, ee))
    eres = float(np.abs(got["residual"] - back).max())
    print(f"one iteration {arm} n={n}: max |angles - fp64| = {err:.3e} degrees, max |residual - fp64 of returned| = {eres:.3e}")
    assert (got["steps"] == 1).all() and np.isfinite(got["angles"]).all()
    assert np.abs(got["angles"] - q0).max() > 1.0
    assert eres <= ik_ref.RESIDUAL_TOL
    assert err <= ik_ref.STEP_TOL


# ---- 3. the settled outcome ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["zero", "random"])
@pytest.mark.parametrize("arm", ["ref", "dh7"])
def test_settled_envs_land_on_their_target(m, arm, kind):
    """32 iterations at the defaults, 4 096 targets of radius 51.3.  For every env the fp64 restatement settles (box
    residual < 1e-3 after 16 and after 32 iterations), the GPU's angles pushed through the fp64 chain must have a box
    residual < 1e-3.  Joint angles are not compared: the redundant arm has several solutions.
    Measured on an MI355X: the largest such residual is 1.607e-05 (the 7-joint arm from random poses; 8.963e-06 .. 1.579e-05
    for the other three cases), and 99.85 - 100 % of ALL envs end below 1e-3."""
    eng = engine(m, arm, ik_ref.SETTLED_N)
    table, ee = ik_ref.arm_table(arm), ik_ref.ARMS[arm][2]
    x, q0 = ik_ref.settled_case(arm, kind)
    settled = ik_ref.settled_reference(arm, kind)
    assert settled.mean() >= ik_ref.SETTLED_SHARE, f"vacuous: only {settled.mean():.4f} of the envs settle in fp64"
    got = solve(eng, x, q0, iters=32, tol=0.0)
    back = ik_ref.box(x.astype(np.float64) - ik_ref.position(got["angles"], table, ee))
    worst = float(back[settled].max())
    print(f"settled {arm} from {kind}: {100 * settled.mean():.2f} % settled, GPU max box residual of those = {worst:.3e}, "
          f"GPU share below 1e-3 overall = {100 * (back < 1e-3).mean():.2f} %")
    assert (got["steps"] == 32).all()
    assert ((got["angles"] >= -180.0) & (got["angles"] < 180.0)).all()         # (wrap is the default)
    assert worst < ik_ref.SETTLED_TOL
    assert np.abs(got["residual"] - back).max() <= ik_ref.RESIDUAL_TOL


# ---- 4. the nearest alive target -----------------------------------------------------------------------------------------
def scattered(m, arm, n, K, tag=0):
    """An engine a few random steps into an episode, some targets and -- for every 9th env -- all of them cleared by hand."""
    eng = engine(m, arm, n, K, tag=tag, pickup_tol=16.0)
    eng.reset_random(SEED + K, 0)
    eng.rollout(4, SEED, 0)
    alive = eng.get(m.lib.F_ALIVE).copy()
    rng = np.random.RandomState(n + K)
    alive[rng.rand(*alive.shape) < 0.3] = 0
    alive[::9] = 0
    eng.set(m.lib.F_ALIVE, alive.astype(np.uint8))
    return eng, alive.astype(bool)


@pytest.mark.parametrize("arm, n, ld, K", [("ref", 600, 600, 7), ("dh7", 200, 256, 7), ("ref_rt", 200, 256, 32), ("rt6_f", 200, 256, 7)])
def test_nearest_alive_target(m, arm, n, ld, K):
    eng, alive = scattered(m, arm, n, K)
    table, ee = ik_ref.arm_table(arm), ik_ref.ARMS[arm][2]
    pts, q0 = eng.points().astype(np.float64), eng.goals()
    assert np.array_equal(eng.get(m.lib.F_ALIVE).astype(bool), alive) and 0 < alive.mean() < 1
    got = solve(eng, None, None, ld, iters=4, wrap=False)
    idx = got["index"]
    none = ~alive.any(axis=1)
    assert none.sum() >= n // 9 and (~none).sum() > n // 2
    assert np.array_equal(idx == -1, none)
    np.testing.assert_array_equal(bits(got["angles"][none]), bits(q0[none]))
    assert (got["residual"][none] == 0).all() and (got["steps"][none] == 0).all() and (got["steps"][~none] == 4).all()
    _, d2 = ik_ref.nearest(pts, alive, q0, table, ee)
    live = np.flatnonzero(~none)
    assert alive[live, idx[live]].all()
    assert (np.sqrt(d2[live, idx[live]]) <= np.sqrt(d2[live].min(axis=1)) + 1e-3).all()
    x = np.zeros((n, 3), dtype=np.float32)
    x[live] = eng.points()[live, idx[live]]
    explicit = solve(eng, x, q0, ld, iters=4, wrap=False)
    for key in ("angles", "residual", "steps"):
        np.testing.assert_array_equal(bits(got[key][live]), bits(explicit[key][live]), err_msg=key)


# ---- 5. staging ----------------------------------------------------------------------------------------------------------
def resident(m, eng):
    L = m.lib
    fields = (L.F_ACTIONS, L.F_GOALS, L.F_POINTS, L.F_ALIVE, L.F_OBS, L.F_REWARD, L.F_DONE, L.F_DONE_BITS, L.F_EE, L.F_TOTAL_REWARD,
              L.F_EPISODES, L.F_LAST_RETURN, L.F_RETURN_RING)
    return {f: eng.get(f).copy() for f in fields}


def same_state(a, b):
    for f in a:
        np.testing.assert_array_equal(bits(a[f]), bits(b[f]), err_msg=f"field {f}")


@pytest.mark.parametrize("arm, n", [("ref", 600), ("dh7", 200), ("rt6_f", 200)])
def test_staged_angles_step_as_set_actions_does(m, arm, n):
    a, alive = scattered(m, arm, n, 7, tag=1)
    b, alive_b = scattered(m, arm, n, 7, tag=2)
    assert np.array_equal(alive, alive_b)
    same_state(resident(m, a), resident(m, b))
    res = a.ik(stage=True, wrap=False)
    a.sync()
    angles = res["angles"].cpu().numpy().T.copy()
    idx, box = res["index"].cpu().numpy(), res["residual"].cpu().numpy()
    np.testing.assert_array_equal(bits(a.get(m.lib.F_ACTIONS)), bits(angles))
    assert np.abs(angles - a.goals()).max() > 1.0
    a.step()
    b.step(angles)
    a.sync(), b.sync()
    same_state(resident(m, a), resident(m, b))
    assert a.bad_action_count() == b.bad_action_count()
    np.testing.assert_array_equal(bits(a.goals()), bits(angles))
    # the pickup the solver aimed for happens: a target whose box residual is inside the pickup box (16, with a guard band) is
    # dead after the step, whatever the route did to the reward
    reached = np.flatnonzero((idx >= 0) & (box < 15.9))
    assert reached.size > n // 2 and not a.alives()[reached, idx[reached]].any()


@pytest.mark.parametrize("arm, n", [("ref", 600), ("rt6_f", 200)])
def test_without_stage_nothing_resident_changes(m, arm, n):
    eng, _ = scattered(m, arm, n, 7, tag=3)
    eng.sample_actions(SEED, 9)
    before = resident(m, eng)
    res = eng.ik()
    J = eng.jacobian(position=True)
    eng.sync()
    assert np.isfinite(res["angles"].cpu().numpy()).all() and np.isfinite(J[0].cpu().numpy()).all()
    same_state(before, resident(m, eng))


# ---- 6. early stop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm, n, ld", [("ref", 600, 600), ("dh7", 200, 256), ("rt6_f", 200, 256)])
def test_early_stop_is_bit_equal_to_a_shorter_run(m, arm, n, ld):
    eng = engine(m, arm, n)
    x, q0 = ik_ref.step_case(arm, n)
    x[:5] = ik_ref.position(q0[:5], ik_ref.arm_table(arm), ik_ref.ARMS[arm][2]).astype(np.float32)   # already there: 0 steps
    got = solve(eng, x, q0, ld, iters=8, tol=1.0, wrap=False)
    steps = got["steps"]
    assert steps.min() == 0 and steps.max() == 8 and len(np.unique(steps)) >= 4, np.unique(steps)
    assert (got["residual"][steps < 8] <= 1.0).all()
    np.testing.assert_array_equal(bits(got["angles"][steps == 0]), bits(q0[steps == 0]))
    for s in range(1, 9):
        short = solve(eng, x, q0, ld, iters=s, tol=0.0, wrap=False)
        sel = steps == s
        np.testing.assert_array_equal(bits(got["angles"][sel]), bits(short["angles"][sel]), err_msg=f"{s} steps")
        np.testing.assert_array_equal(bits(got["residual"][sel]), bits(short["residual"][sel]), err_msg=f"{s} steps")


# ---- 7. wrap -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm, n, ld", [("ref", 600, 600), ("dh7", 200, 256)])
def test_wrapped_angles_are_the_same_pose(m, arm, n, ld):
    eng = engine(m, arm, n)
    x, q0 = ik_ref.step_case(arm, n)
    q0 = q0 + np.float32(360.0) * np.arange(-2, 3, dtype=np.float32)[np.arange(n) % 5][:, None]   # starts up to +-900 degrees
    plain = solve(eng, x, q0, ld, iters=6, wrap=False)
    wrapped = solve(eng, x, q0, ld, iters=6, wrap=True)
    w = wrapped["angles"]
    assert ((w >= -180.0) & (w < 180.0)).all() and (np.abs(plain["angles"]) >= 180.0).mean() > 0.5
    turns = (plain["angles"].astype(np.float64) - w) / 360.0
    assert np.abs(turns - np.rint(turns)).max() * 360.0 <= 1e-4
    assert np.abs(wrapped["residual"] - plain["residual"]).max() <= 1e-3
    np.testing.assert_array_equal(wrapped["steps"], plain["steps"])


# ---- 8. bounds, determinism, poison --------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm, n, ld", [("ref", 200, 256), ("rt8", 600, 600)])
def test_two_calls_and_a_graph_replay_give_the_same_bits(m, arm, n, ld):
    import torch
    eng = engine(m, arm, n)
    x, q0 = ik_ref.step_case(arm, n)
    want = solve(eng, x, q0, ld, iters=5)
    again = solve(eng, x, q0, ld, iters=5)
    for key in want:
        np.testing.assert_array_equal(bits(want[key]), bits(again[key]), err_msg=key)
    dev = torch.device("cuda", eng.device)
    xd, qd = rows_in(eng, x, ld), rows_in(eng, q0, ld)
    ang = torch.zeros((eng.dof, n), dtype=torch.float32, device=dev)
    res, stp = torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    try:
        with torch.cuda.stream(side):
            eng.use_torch_stream()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                eng.ik(xd, qd, iters=5, angles=ang, residual=res, steps=stp)
        torch.cuda.synchronize(dev)
        assert not ang.cpu().numpy().any()                       # captured, not run
        for r in range(2):
            ang.fill_(3.0)
            graph.replay()
            torch.cuda.synchronize(dev)
            np.testing.assert_array_equal(bits(ang.cpu().numpy().T), bits(want["angles"]), err_msg=f"replay {r}")
            np.testing.assert_array_equal(bits(res.cpu().numpy()), bits(want["residual"]), err_msg=f"replay {r}")
            np.testing.assert_array_equal(stp.cpu().numpy(), want["steps"])
    finally:
        eng.set_stream(None)                                     # the engine is shared: back to its own stream


@pytest.mark.parametrize("arm, n, ld", [("ref", 200, 256), ("dh7", 600, 600), ("rt6_f", 200, 256)])
def test_poisoned_envs_are_held_and_change_no_neighbour(m, arm, n, ld):
    eng = engine(m, arm, n)
    x, q0 = ik_ref.step_case(arm, n)
    clean = solve(eng, x, q0, ld, iters=5, tol=0.5)
    xp, qp = x.copy(), q0.copy()
    xp[3, 1], xp[70, 0], qp[64, 0], qp[130, eng.dof - 1], qp[199, 1] = np.nan, np.inf, np.inf, np.nan, 40000.0
    bad = np.zeros(n, dtype=bool)
    bad[[3, 70, 64, 130, 199]] = True
    got = solve(eng, xp, qp, ld, iters=5, tol=0.5)
    np.testing.assert_array_equal(bits(got["angles"][bad]), bits(qp[bad]))
    assert np.isnan(got["residual"][bad]).all() and (got["steps"][bad] == 0).all()
    for key in clean:
        np.testing.assert_array_equal(bits(got[key][~bad]), bits(clean[key][~bad]), err_msg=key)
    assert np.isfinite(got["residual"][~bad]).all()


def test_reach_actions_in_the_reference_loop(m):
    env = m.Multienv(env_shape=(1, 6), obj_number=5)
    env.reset()
    act = env.reach_actions()
    assert len(act) == 6 and len(act[0]) == 4
    obs, rew, done = env.step(act)
    assert len(rew) == 6 and (env.engine.alives().sum(axis=1) <= 4).all()      # every arm picked its nearest target up
    env.close()
    env = m.Multienv(env_shape=(2, 300), obj_number=5, rng="device")
    env.reset()
    assert env.reach_actions() is env.DEVICE_ACTIONS
    env.step(env.DEVICE_ACTIONS)
    assert (env.engine.alives().sum(axis=1) <= 4).mean() >= 0.98
    env.close()


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(m):
    import torch
    L = m.lib
    n = 200
    eng = m.StepEngine(n, 7)
    dev = torch.device("cuda", eng.device)
    x, q0 = ik_ref.step_case("ref", n)
    xd, qd = rows_in(eng, x, n), rows_in(eng, q0, n)
    ang = torch.zeros((4, n), dtype=torch.float32, device=dev)
    idx = torch.zeros(n, dtype=torch.int32, device=dev)

    def arg(**over):
        s = L.MtIk()
        s.struct_size = C.sizeof(s)
        s.iters, s.damping, s.max_step_deg, s.tol, s.flags = 4, 2.0, 30.0, 0.0, L.IK_WRAP
        s.target, s.target_ld, s.start, s.start_ld = xd.data_ptr(), n, qd.data_ptr(), n
        s.angles_out, s.angles_ld = ang.data_ptr(), n
        for k, v in over.items():
            setattr(s, k, v)
        return s

    def call(**over):
        torch.cuda.synchronize(dev)
        return eng._lib.mt_ik(eng._h, C.byref(arg(**over)))

    def good():
        ang.zero_()
        assert call() == L.MT_OK
        eng.sync()
        assert ang.cpu().numpy().any()

    good()                                                       # explicit target and start: no resident state, no reset needed
    for over in (dict(target=None), dict(start=None), dict(flags=L.IK_STAGE)):
        assert call(**over) == L.MT_ERR_STATE, over
        assert b"reset" in eng._lib.mt_last_error(eng._h)
        good()
    assert eng._lib.mt_jacobian(eng._h, None, 0, ang.data_ptr(), n, None, 0) == L.MT_ERR_STATE
    eng.reset_random(SEED, 0)
    for over in (dict(iters=0), dict(iters=256), dict(damping=0.0), dict(damping=float("nan")), dict(target_ld=n - 1),
                 dict(start_ld=n - 1), dict(angles_ld=n - 1), dict(index_out=idx.data_ptr()), dict(angles_out=None),
                 dict(flags=4), dict(max_step_deg=float("inf")), dict(tol=-1.0), dict(reserved=1)):
        assert call(**over) == L.MT_ERR_INVALID_ARG, over
        good()
    assert call(target=None, index_out=idx.data_ptr()) == L.MT_OK
    with pytest.raises(ValueError):
        eng.ik(xd, index=True)
    with pytest.raises(ValueError):
        eng.ik(angles=False, residual=False, index=False)
    with pytest.raises(ValueError):
        eng.ik(iters=256)
    with pytest.raises(ValueError):
        eng.ik(xd[:, :100])
    jac = torch.zeros((12, n), dtype=torch.float32, device=dev)
    assert eng._lib.mt_jacobian(eng._h, qd.data_ptr(), n - 1, jac.data_ptr(), n, None, 0) == L.MT_ERR_INVALID_ARG
    assert eng._lib.mt_jacobian(eng._h, qd.data_ptr(), n, jac.data_ptr(), n - 1, None, 0) == L.MT_ERR_INVALID_ARG
    assert eng._lib.mt_jacobian(eng._h, qd.data_ptr(), n, None, n, None, 0) == L.MT_ERR_INVALID_ARG
    assert eng._lib.mt_jacobian(eng._h, qd.data_ptr(), n, jac.data_ptr(), n, None, 0) == L.MT_OK
    good()
    eng.close()
    origin = m.StepEngine(n, 7, ee_frame=-4)
    origin.reset_random(SEED, 0)
    with pytest.raises(m.ManytorError) as e:
        origin.ik()
    assert e.value.status == L.MT_ERR_UNSUPPORTED
    with pytest.raises(m.ManytorError) as e:
        origin.jacobian()
    assert e.value.status == L.MT_ERR_UNSUPPORTED
    origin.step_random(SEED, 0)                                  # the handle stays usable
    origin.sync()
    origin.close()
