"""GPU tests of the target codes: the prefetch step kernels read each target as its 8-byte draw code while the handle knows the
codes to match MT_F_POINTS.  A handle on codes and a handle forced onto the floats (mt_device_ptr(MT_F_POINTS) before its first
step) run the same scripts and must agree bit for bit in every field -- across the writers that keep the codes (full random
resets, the re-arm of finished envs, the code-reading steps) and those that end them (mt_set, checkpoint restore, the fused
rollout)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("F_GOALS", "F_ALIVE", "F_TOTAL_REWARD", "F_POINTS", "F_EPISODES", "F_LAST_RETURN", "F_OBS", "F_REWARD", "F_DONE",
          "F_EE", "F_DONE_BITS", "F_RETURN_RING")
SEED = 0xC0DE
K = 7
TOL = 30.0  # a wide pickup box: targets get picked, and dead ones zeroed, every few steps


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32) if v.dtype == np.float32 else v


def assert_same(m, got, want, what):
    for f in FIELDS:
        a, b = got.get(getattr(m.lib, f)), want.get(getattr(m.lib, f))
        assert a.dtype == b.dtype, (what, f)
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"{what}: {f}")


def pair(m, n):
    codes = m.StepEngine(n, K, pickup_tol=TOL)
    floats = m.StepEngine(n, K, pickup_tol=TOL)
    floats.device_ptr(m.lib.F_POINTS)  # the floats from now on, for good
    return codes, floats


def episodes(e, first, count, steps=20):
    for ep in range(first, first + count):
        e.reset_random(SEED, ep)
        e.rollout(steps, SEED, ep * steps)


@pytest.mark.parametrize("n", [1048576, 300007, 4194304])
def test_codes_and_floats_agree_over_episodes(m, n):
    codes, floats = pair(m, n)
    try:
        for ep in range(3):
            for e in (codes, floats):
                episodes(e, ep, 1)
                e.sync()
            assert_same(m, codes, floats, f"n={n} episode {ep}")
        # some targets were picked and zeroed, and some envs finished
        pts = codes.points()
        assert (pts == 0).all(axis=2).any() and codes.done().any()
        for e in (codes, floats):
            e.reset_done(SEED)
            e.rollout(7, SEED, 100)
            e.sync()
        assert_same(m, codes, floats, f"n={n} reset_done")
    finally:
        codes.close()
        floats.close()


def run_pair(m, n, script):
    codes, floats = pair(m, n)
    try:
        for e in (codes, floats):
            script(e)
            e.sync()
        assert_same(m, codes, floats, script.__name__)
    finally:
        codes.close()
        floats.close()


def test_set_points_then_steps(m):
    rng = np.random.default_rng(7)
    pts = rng.uniform(-40.0, 40.0, size=(1048576, K, 3)).astype(np.float32)
    pts[..., 2] = np.abs(pts[..., 2])

    def set_points(e):
        episodes(e, 0, 1, steps=3)
        e.set(m.lib.F_POINTS, pts)
        e.rollout(6, SEED, 3)
        episodes(e, 1, 1, steps=6)  # a full reset brings the codes back

    run_pair(m, 1048576, set_points)


def test_reset_done_between_steps(m):
    def rearm(e):
        episodes(e, 0, 1, steps=12)
        for s in range(3):
            e.reset_done(SEED)
            e.rollout(4, SEED, 12 + 4 * s)

    run_pair(m, 1048576, rearm)


def test_fused_rollout_then_steps(m):
    def fused(e):
        episodes(e, 0, 1, steps=4)
        e.rollout_fused(5, SEED, 4, auto_reset=True)
        e.rollout(6, SEED, 9)
        episodes(e, 1, 1, steps=5)

    run_pair(m, 1048576, fused)


def test_per_chain_reset_while_forked(m):
    def forked(e):
        assert e.dispatch()["chains"]["count"] > 1
        e.reset_random(SEED, 0)
        e.rollout(5, SEED, 0)          # leaves the chains forked
        e.reset_random(SEED, 1)        # one reset per chain, behind that chain's last step
        e.rollout(5, SEED, 5)
        e.reset_done(SEED)             # whole batch, right behind per-chain work
        e.rollout(5, SEED, 10)

    run_pair(m, 1048576, forked)


def test_checkpoint_restore(m):
    def restore(e):
        episodes(e, 0, 1, steps=6)
        st = e.get_state()
        e.rollout(5, SEED, 6)
        e.set_state(st)
        e.rollout(8, SEED, 6)

    run_pair(m, 1048576, restore)
