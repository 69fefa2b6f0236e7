"""shoot_kernel, cem_kernel and mppi_kernel share one step (plan_step), one block prologue (plan_start) and one refit head
(refit_head).  The three must agree bit for bit on one block of plans at the shapes where those shared pieces can go wrong
and that the planners' own files leave open:

  n = 1    : a lone live lane in a block of tail lanes;      n = 65 : one full wave plus a block of one lane
  K = 1    : the smallest target tile;                       K = 32 : the largest, the score tile at its largest offset
  T = 1    : only wave 0 refits, no pose cache carried over; T = 3  : three waves refit, the cache is carried
  C = 1, 3 : three idle waves, one idle wave;                C = 6  : two waves with two candidates each

Per case: a fresh handle, reset_random, sample_plans() into the (C, T, D, n) block, shoot() on the block, cem() and mppi()
with the same mean / sigma / seed / draw, both committing H = T steps (mppi on a twin handle: a commit moves the state).
`candidate_returns`, `best` and `best_return` are compared as int32 views; `chosen` of cem and of mppi is the best plane of
the block.  The inputs are test_gpu_cem's shaped moments: sigma up to 60 degrees, so the candidates of an env differ.
"""
import numpy as np
import pytest

from test_gpu_cem import PLAN_SEED, dev, shaped_moments
from test_gpu_shoot import host
from test_gpu_tape import SEED, _table, make_engine

pytestmark = pytest.mark.gpu

TOL = {"ref": 20.0, "dh7": 45.0, "rt5": 20.0}


@pytest.fixture(scope="module")
def m():
    import manytor_amd
    if manytor_amd.device_count() < 1:
        pytest.fail("gpu tests need a visible MI355X and the in-tree libmanytor_hip.so")
    return manytor_amd


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("C_", (1, 3, 6), ids=lambda v: f"C{v}")
@pytest.mark.parametrize("T", (1, 3), ids=lambda v: f"T{v}")
@pytest.mark.parametrize("k", (1, 32), ids=lambda v: f"K{v}")
@pytest.mark.parametrize("n", (1, 65), ids=lambda v: f"n{v}")
@pytest.mark.parametrize("table_name", ("ref", "dh7", "rt5"))
def test_shoot_cem_and_mppi_agree_on_the_sampled_block(m, table_name, n, k, T, C_):
    D = len(_table(m, table_name)[0])
    mean, sigma = shaped_moments(T, n, D)
    keep = T == 3 and C_ == 6                                      # candidate 0 is the clamped mean: plan_angles' other branch
    kw = dict(candidates=C_, draw=3, seed=PLAN_SEED, keep_mean=keep)
    a, b = (make_engine(m, table_name, n, k, TOL[table_name]) for _ in range(2))
    for eng in (a, b):
        eng.reset_random(SEED, 0)
    mean_a, sigma_a, mean_b, sigma_b = dev(a, mean), dev(a, sigma), dev(b, mean), dev(b, sigma)
    block = a.sample_plans(mean_a, sigma_a, **kw)
    shoot = host(a.shoot(block, all_returns=True))
    cem = host(a.cem(mean_a, sigma_a, elites=1, commit=T, all_returns=True, **kw))
    mppi = host(b.mppi(mean_b, sigma_b, decay=0.5, commit=T, all_returns=True, **kw))
    block = block.cpu().numpy()
    distinct = np.unique(shoot["candidate_returns"])
    print(f"[planners-agree] {table_name} n={n} K={k} T={T} C={C_} keep_mean={keep}: distinct returns {distinct.tolist()}")
    assert shoot["candidate_returns"].shape == (C_, n)
    if n == 65:
        assert len(distinct) >= 2, distinct                        # equal constants would prove nothing
    for name, got in (("cem", cem), ("mppi", mppi)):
        for key in ("candidate_returns", "best", "best_return"):
            assert got[key].dtype == shoot[key].dtype and got[key].shape == shoot[key].shape
            np.testing.assert_array_equal(bits(got[key]), bits(shoot[key]), err_msg=f"{name} {key}")
        best_plane = block[shoot["best"], :, :, np.arange(n)].transpose(1, 2, 0)            # (T, D, n)
        np.testing.assert_array_equal(bits(got["chosen"]), bits(best_plane), err_msg=f"{name} chosen")
    a.close()
    b.close()
