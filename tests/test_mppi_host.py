"""CPU-only checks of mt_mppi's host side: the symbol is exported, the ctypes mirror of struct mt_mppi has the C struct's
layout, the restated table and refit (tests/mppi_ref.py) give the exact values the header's definitions give by hand, and
StepEngine.mppi refuses what it can refuse before it touches the library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mppi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("struct_size", "n_steps", "n_candidates", "commit_steps", "draw", "decay", "mean", "sigma", "ld", "mean_out",
          "sigma_out", "out_ld", "lo", "hi", "sigma_min", "returns_out", "ret_ld", "weights_out", "w_ld", "weight_sum_out",
          "best_out", "best_return_out", "chosen_out", "chosen_ld", "reward_log", "done_log", "log_ld", "return_out", "seed",
          "flags", "reserved")


@pytest.fixture(scope="module")
def lib():
    from manytor_amd import build, _lib
    build.build_library()            # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_mppi_is_exported_and_prototyped(lib):
    from manytor_amd import _lib
    assert hasattr(lib, "mt_mppi")
    res, args = _lib.PROTOTYPES["mt_mppi"]
    assert res is ctypes.c_int and args == [_lib._HANDLE, ctypes.POINTER(_lib.MtMppi)]
    assert lib.mt_version() >= 430


def test_ctypes_mppi_matches_c_layout(lib, tmp_path):
    from manytor_amd import _lib
    src = tmp_path / "mppi_sz.c"
    offsets = ", ".join(f"offsetof(struct mt_mppi,{f})" for f in FIELDS)
    fmt = " ".join(["%zu"] * (len(FIELDS) + 1))
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "manytor_hip.h"\n'
        f'int main(void){{printf("{fmt} %u %u %d\\n", sizeof(struct mt_mppi), {offsets}, MT_MPPI_AUTO_RESET, MT_MPPI_KEEP_MEAN,'
        ' MT_MPPI_MAX_STEPS);return 0;}\n')
    exe = tmp_path / "mppi_sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _lib.MtMppi
    assert [name for name, _ in S._fields_] == list(FIELDS)
    assert c == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + [_lib.MPPI_AUTO_RESET, _lib.MPPI_KEEP_MEAN,
                                                                              _lib.MPPI_MAX_STEPS]
    assert _lib.MPPI_MAX_STEPS == mppi_ref.MAX_STEPS == 127


def test_null_handle_is_an_invalid_argument(lib):
    from manytor_amd import _lib
    s = _lib.MtMppi()
    s.struct_size = ctypes.sizeof(_lib.MtMppi)
    assert lib.mt_mppi(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)
    assert lib.mt_mppi(None, None) == _lib.MT_ERR_INVALID_ARG


def test_restated_table():
    T = 127
    np.testing.assert_array_equal(mppi_ref.table(1.0, T), np.ones(2 * T + 1, dtype=np.float32))
    hard = mppi_ref.table(0.0, T)
    assert hard.dtype == np.float32 and hard[0] == 1 and (hard[1:] == 0).all()
    half = mppi_ref.table(0.5, T)                                  # 2^-k down to 2^-254: exact, the tail subnormal
    np.testing.assert_array_equal(half.astype(np.float64)[:150], np.ldexp(1.0, -np.arange(150)))
    assert half[126] == np.float32(2.0 ** -126) and half[149] == np.float32(2.0 ** -149) and (half[150:] == 0).all()
    for rho in (0.25, float(mppi_ref.decay_of(1.5)), 0.9990234375, float(mppi_ref.decay_of(0.05))):
        w = mppi_ref.table(rho, T)
        assert w.shape == (2 * T + 1,) and w[0] == 1 and w[1] == np.float32(rho)
        assert (np.diff(w) <= 0).all() and (w >= 0).all()          # monotone: no entry above its predecessor
        exact = np.float64(np.float32(rho)) ** np.arange(2 * T + 1)
        normal = exact > 1e-37
        assert np.abs(w[normal] / exact[normal] - 1).max() < 2 * T * 2.0 ** -24      # k roundings of half an ulp each
    assert mppi_ref.decay_of(1.5).dtype == np.float32 and abs(float(mppi_ref.decay_of(1.5)) - 0.5134171) < 1e-7


def test_restated_gap_weights_and_refit_on_a_hand_made_case():
    """C = 4, n = 3, T = D = 1, decay = 0.5: every product and sum below is exact in fp32, so the expected values are too."""
    returns = np.array([[1, -1, 0], [1, 0, 0], [-1, 1, 0], [0, 1, 0]], dtype=np.float32)
    np.testing.assert_array_equal(mppi_ref.gaps(returns), [[0, 2, 0], [0, 1, 0], [2, 0, 0], [1, 0, 0]])
    b, br = mppi_ref.best(returns)
    np.testing.assert_array_equal(b, [0, 2, 0])                    # the lowest index wins the tie
    np.testing.assert_array_equal(br, [1, 1, 0])
    w = mppi_ref.weights(returns, 0.5, 1)
    assert w.dtype == np.float32
    np.testing.assert_array_equal(w, [[1, .25, 1], [1, .5, 1], [.25, 1, 1], [.5, 1, 1]])
    np.testing.assert_array_equal(mppi_ref.weight_sum(w), [2.75, 2.75, 4])
    plans = np.array([[8, 4, 1], [-8, 8, 3], [16, 2, 5], [4, -2, 7]], dtype=np.float32).reshape(4, 1, 1, 3)
    m, s = mppi_ref.refit(plans, w, 0.0)
    # env 0: A = 8 - 8 + 4 + 2 = 6; env 1: A = 1 + 4 + 2 - 2 = 5; env 2: the plain average of 1, 3, 5, 7
    want_m = np.array([6, 5, 16], dtype=np.float32) / np.array([2.75, 2.75, 4], dtype=np.float32)
    np.testing.assert_array_equal(m[0, 0], want_m)
    assert m[0, 0, 2] == 4 and s[0, 0, 2] == np.float32(np.sqrt(np.float32(5)))      # deviations 3, 1, 1, 3: Q / S = 20 / 4
    assert mppi_ref.refit(plans, w)[1] is None
    np.testing.assert_array_equal(mppi_ref.refit(plans, w)[0], m)
    np.testing.assert_array_equal(mppi_ref.refit(plans, w, 100.0)[1], np.full((1, 1, 3), 100, dtype=np.float32))
    # the hard maximum: only the candidates tied with the best count
    hard = mppi_ref.weights(returns, 0.0, 1)
    np.testing.assert_array_equal(hard, [[1, 0, 1], [1, 0, 1], [0, 1, 1], [0, 1, 1]])
    m0, s0 = mppi_ref.refit(plans, hard, 0.0)
    np.testing.assert_array_equal(m0[0, 0], [0, 0, 4])
    np.testing.assert_array_equal(s0[0, 0], [8, 2, np.float32(np.sqrt(np.float32(5)))])


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched: {name}")


def test_python_front_end_refuses_before_it_touches_the_library(lib):
    """An engine object without a handle: every refusal below has to come from the argument checks alone."""
    import torch
    from manytor_amd.engine import StepEngine
    n, d, T = 10, 4, 3
    eng = object.__new__(StepEngine)
    eng.n_envs, eng.dof, eng.device, eng.version = n, d, 0, 0
    eng._lib = eng._h = _Untouchable()
    host = torch.zeros((T, d, n), dtype=torch.float32)
    kw = dict(candidates=4, decay=0.5)
    with pytest.raises(ValueError, match="CUDA float32"):
        eng.mppi(host, host, **kw)                                             # host tensors are not read in place
    with pytest.raises(ValueError, match="CUDA float32"):
        eng.mppi(np.zeros((T, d, n), dtype=np.float32), host, **kw)
    with pytest.raises(ValueError, match="CUDA float32"):
        eng.mppi(host, host, candidates=4, temperature=1.5)
    for c in (0, 65):
        with pytest.raises(ValueError, match="candidates"):
            eng.mppi(host, host, **dict(kw, candidates=c))
    long = torch.zeros((128, d, n), dtype=torch.float32)
    with pytest.raises(ValueError, match="at most 127 steps"):
        eng.mppi(long, long, **kw)                                             # T > 127
    with pytest.raises(ValueError, match="exactly one of temperature and decay"):
        eng.mppi(host, host, candidates=4)
    with pytest.raises(ValueError, match="exactly one of temperature and decay"):
        eng.mppi(host, host, candidates=4, temperature=1.0, decay=0.5)
    for bad in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="decay"):
            eng.mppi(host, host, candidates=4, decay=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            eng.mppi(host, host, candidates=4, temperature=bad)
    for lo, hi in ((float("nan"), 1.0), (-1.0, float("inf")), (2.0, 1.0), (-40000.0, 0.0)):
        with pytest.raises(ValueError, match="lo <= hi"):
            eng.mppi(host, host, lo=lo, hi=hi, **kw)
    for bad in (float("nan"), -1.0, float("inf")):
        with pytest.raises(ValueError, match="sigma_min"):
            eng.mppi(host, host, sigma_min=bad, **kw)
    with pytest.raises(ValueError, match="auto_reset"):
        eng.mppi(host, host, auto_reset=True, **kw)                            # nothing to re-arm without a commit
    assert eng.version == 0
