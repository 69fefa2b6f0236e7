"""GPU tests of the block-cooperative ground test (kernels.h GroundQueue, step_kernel<.., GC>): the interior poses of a
route are evaluated only for the envs whose two end poses clear the ground, on dense lanes of the block.  It is the same
arithmetic on the same inputs in another lane, so a default engine and an MT_GROUND_COMPACT=0 engine (the per-lane loop)
must agree bit for bit in every state and step field, whatever the number of undecided envs in a block -- none, one in a
partial block, more than the queue holds -- and the ground flag itself is held to the fp64 oracle on routes that touch
the ground at interior poses only.

Every script runs on the engines mt_create picks for the size (the lane-split and multi-step forms of the small batches
never take the queue: those cases pin that the switch changes nothing there), and with MT_SPLIT=1 MT_ROLLOUT_K=1, which
puts the one-env-per-lane step kernels -- the kernels of the large batches -- on every size: with the prefetch the policy
picks, in the flat addressing of the largest launches, and without prefetch."""
import numpy as np
import pytest

from parity_util import GUARD

pytestmark = pytest.mark.gpu

FIELDS = ("F_GOALS", "F_ALIVE", "F_TOTAL_REWARD", "F_POINTS", "F_OBS", "F_REWARD", "F_DONE", "F_EE", "F_DONE_BITS",
          "F_LAST_RETURN")
SEED = 0x6C0DE
RT5 = [[0, -1.2, 5, 0], [6, 0.37, 0, 0.2], [0, 1.57, 7, 0], [4, 0, 0, 0], [3, -1.57, 2, 0]]
ONE_ENV_PER_LANE = {"MT_SPLIT": "1", "MT_ROLLOUT_K": "1"}
MODES = {"default": {}, "one_env_per_lane": ONE_ENV_PER_LANE, "flat": {**ONE_ENV_PER_LANE, "MT_FLAT_FROM": "0"},
         "no_prefetch": {**ONE_ENV_PER_LANE, "MT_PREFETCH": "0"}}


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def table_of(m, name):
    return {"ref": (m.REF_DH_TABLE, 51.3), "dh7": (m.DH7_TABLE, 92.6), "rt5": (RT5, 51.3)}[name]


def bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint32) if v.dtype == np.float32 else v


def assert_same(m, got, want, what, fields=FIELDS):
    for f in fields:
        a, b = got.get(getattr(m.lib, f)), want.get(getattr(m.lib, f))
        assert a.dtype == b.dtype, (what, f)
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"{what}: {f}")


def pair(m, monkeypatch, mode, n, k, table_name, **kw):
    """(default engine, MT_GROUND_COMPACT=0 engine); the overrides are read once, by mt_create."""
    table, radius = table_of(m, table_name)
    for name in MODES["flat"].keys() | MODES["no_prefetch"].keys():
        monkeypatch.delenv(name, raising=False)
    for name, value in MODES[mode].items():
        monkeypatch.setenv(name, value)
    monkeypatch.delenv("MT_GROUND_COMPACT", raising=False)
    on = m.StepEngine(n, k, dh_table=table, radius=radius, **kw)
    monkeypatch.setenv("MT_GROUND_COMPACT", "0")
    off = m.StepEngine(n, k, dh_table=table, radius=radius, **kw)
    monkeypatch.delenv("MT_GROUND_COMPACT", raising=False)
    d_on, d_off = on.dispatch(), off.dispatch()
    assert d_on["ground_compact"]["enabled"] and not d_off["ground_compact"]["enabled"]
    assert not d_off["ground_compact"]["step"] and not d_off["ground_compact"]["chains"]
    assert "MT_GROUND_COMPACT=0" in d_off["overrides"] and "MT_GROUND_COMPACT" not in d_on["overrides"]
    if mode != "default":  # the kernel under test really runs (the long arms keep the per-lane loop), unless MT_F_ZMIN is on
        assert d_on["step"]["lanes_per_env"] == 1 and d_on["rollout"]["steps_per_launch"] == 1
        want = table_name != "dh7" and not kw.get("debug_zmin", False)
        assert d_on["ground_compact"]["step"] == want and d_on["ground_compact"]["chains"] == want
    return on, off


def run_pair(m, on, off, script, what):
    try:
        for e in (on, off):
            script(e)
            e.sync()
        assert_same(m, on, off, what)
    finally:
        on.close()
        off.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("table_name", ["ref", "dh7", "rt5"])
@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("n", [300, 769, 5000, 70001])
def test_ragged_sizes_agree_with_the_per_lane_loop(m, monkeypatch, n, k, table_name, mode):
    on, off = pair(m, monkeypatch, mode, n, k, table_name, pickup_tol=30.0)

    def script(e):
        e.reset_random(SEED, 0)
        e.step_random(SEED, 0)  # from the zero pose: about half of the envs are undecided
        e.rollout(9, SEED, 1)
        e.reset_done(SEED)
        e.rollout(4, SEED, 10)

    run_pair(m, on, off, script, f"n={n} K={k} {table_name} {mode}")


def _below_ground_action(m):
    """A whole-degree action of the reference arm whose END pose has a frame well below ground (fp64 oracle)."""
    from oracle.manytor_oracle import batch_joints_coordinates
    rng = np.random.default_rng(11)
    cand = rng.integers(-180, 180, size=(512, 4)).astype(np.float64)
    jc = batch_joints_coordinates(cand, np.asarray(m.REF_DH_TABLE))
    z = np.minimum(jc[:, -2, 2], jc[:, -1, 2])
    return cand[np.argmin(z)].astype(np.float32), float(z.min())


STAGED = ["all_zero_pose", "all_below_ground", "one_undecided_in_partial_block", "terminate_on_ground", "one_wide_lane"]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", STAGED)
def test_staged_actions_agree_with_the_per_lane_loop(m, monkeypatch, case, mode):
    n, k = 769, 7  # three whole blocks and a block of one env
    rng = np.random.default_rng(5)
    down, z_down = _below_ground_action(m)
    assert z_down < -1.0
    rand = rng.integers(-180, 180, size=(n, 4)).astype(np.float32)
    if case == "all_zero_pose":  # every env undecided: twice what the queue holds, the rest walk their own routes
        acts = np.zeros((n, 4), np.float32)
    elif case == "all_below_ground":  # an empty queue
        acts = np.tile(down, (n, 1))
    elif case == "one_undecided_in_partial_block":
        acts = np.tile(down, (n, 1))
        acts[n - 1] = 0.0
    elif case == "terminate_on_ground":
        acts = rand
    else:  # one lane of one wave beyond +-180: that wave takes the wide form, and still serves the block's queue
        acts = rand.copy()
        acts[70, 1] = 540.0
    on, off = pair(m, monkeypatch, mode, n, k, "ref", pickup_tol=30.0, terminate_on_ground=(case == "terminate_on_ground"))

    def script(e):
        e.reset_random(SEED, 0)
        e.step(acts)
        e.step(rand[::-1].copy())  # and on from the poses that left behind

    run_pair(m, on, off, script, f"staged {case} {mode}")


def test_interior_only_contact_against_the_fp64_oracle(m, monkeypatch):
    """Routes whose two end poses clear the ground by more than the guard and whose interior dips below it by more than
    the guard: decided by the queued poses alone.  Counted and classified by the fp64 oracle; the GPU must give every one
    of them reward -1, and no -1 to an env whose whole route clears the ground by the guard."""
    from oracle.manytor_oracle import batch_joints_coordinates
    n, k, S = 4096, 3, 25
    table = np.asarray(m.REF_DH_TABLE)
    rng = np.random.default_rng(2026)
    prev = rng.integers(-180, 180, size=(n, 4)).astype(np.float64)
    act = rng.integers(-180, 180, size=(n, 4)).astype(np.float64)
    step = (act - prev) / (S - 1)
    z = np.empty((S, n))
    for s in range(S):
        jc = batch_joints_coordinates(act if s == S - 1 else prev + s * step, table)
        z[s] = np.minimum(jc[:, -2, 2], jc[:, -1, 2])
    z_ends, z_int, z_all = np.minimum(z[0], z[-1]), z[1:-1].min(axis=0), z.min(axis=0)
    interior_only = (z_ends > GUARD) & (z_int < -GUARD)
    clear = z_all > GUARD
    in_band = np.abs(z_all) <= GUARD  # the flag itself is not compared there
    assert interior_only.sum() >= 30, int(interior_only.sum())
    assert in_band.sum() < 2e-3 * n + 8, int(in_band.sum())

    for name, value in ONE_ENV_PER_LANE.items():
        monkeypatch.setenv(name, value)
    monkeypatch.delenv("MT_GROUND_COMPACT", raising=False)
    eng = m.StepEngine(n, k, substeps=S, pickup_tol=0.01)
    try:
        assert eng.dispatch()["ground_compact"]["step"]
        eng.reset_random(SEED, 0)
        eng.set(m.lib.F_GOALS, prev.astype(np.float32))
        eng.step(act.astype(np.float32))
        rew = eng.reward()
        print(f"interior-only routes {int(interior_only.sum())}, clear {int(clear.sum())}, in the guard band {int(in_band.sum())}")
        assert (rew[interior_only] == -1).all()
        assert (rew[clear] != -1).all()
        assert (rew[z_all < -GUARD] == -1).all()
    finally:
        eng.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_debug_zmin_keeps_every_pose(m, monkeypatch, mode):
    """MT_F_ZMIN is the minimum over ALL poses of every env: a handle with debug_zmin keeps the per-lane loop, and says so."""
    n = 70001
    on, off = pair(m, monkeypatch, mode, n, 7, "ref", debug_zmin=True)
    try:
        g = on.dispatch()["ground_compact"]
        assert g["enabled"] and not g["step"] and not g["chains"]
        for e in (on, off):
            e.reset_random(SEED, 0)
            e.step_random(SEED, 0)
            e.step_random(SEED, 1)
            e.sync()
        assert_same(m, on, off, "debug_zmin", FIELDS + ("F_ZMIN",))
    finally:
        on.close()
        off.close()


@pytest.mark.parametrize("table_name", ["ref", "rt5"])
@pytest.mark.parametrize("substeps", [2, 3, 24, 26])
def test_other_substep_counts(m, monkeypatch, substeps, table_name):
    """S = 25 has one forward pose more than backward poses.  An even S has as many of each (the `mine` bound of the shared
    loop never bites), S = 3 one forward pose and no backward one, S = 2 no interior pose at all (the queue is filled and
    nothing is walked); S = 26 is the longest route of the recurrence.  The staged zero-pose step leaves every env undecided,
    so the lanes that find the queue full walk their own halves with the same counts."""
    n = 769
    on, off = pair(m, monkeypatch, "one_env_per_lane", n, 7, table_name, pickup_tol=30.0, substeps=substeps)
    dof = len(table_of(m, table_name)[0])

    def script(e):
        e.reset_random(SEED, 0)
        e.step_random(SEED, 0)
        e.rollout(5, SEED, 1)
        e.step(np.zeros((n, dof), np.float32))
        e.step(np.zeros((n, dof), np.float32))  # zero pose to zero pose: a whole block undecided
        e.rollout(3, SEED, 8)

    run_pair(m, on, off, script, f"S={substeps} {table_name}")
