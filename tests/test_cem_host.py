"""CPU-only checks of mt_cem's host side: the symbols are exported, the ctypes mirror of struct mt_cem has the C struct's
layout, the restated noise (tests/cem_ref.py) has the moments the header states, and StepEngine.cem / sample_plans refuse
what they can refuse before they touch the library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cem_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("struct_size", "n_steps", "n_candidates", "n_elites", "commit_steps", "draw", "mean", "sigma", "ld", "mean_out",
          "sigma_out", "out_ld", "lo", "hi", "sigma_min", "returns_out", "ret_ld", "best_out", "best_return_out",
          "elite_mask_out", "chosen_out", "chosen_ld", "reward_log", "done_log", "log_ld", "return_out", "seed", "flags",
          "reserved")


@pytest.fixture(scope="module")
def lib():
    from manytor_amd import build, _lib
    build.build_library()            # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_cem_is_exported_and_prototyped(lib):
    from manytor_amd import _lib
    assert hasattr(lib, "mt_cem") and hasattr(lib, "mt_sample_plans")
    res, args = _lib.PROTOTYPES["mt_cem"]
    assert res is ctypes.c_int and args == [_lib._HANDLE, ctypes.POINTER(_lib.MtCem)]
    res, args = _lib.PROTOTYPES["mt_sample_plans"]
    assert res is ctypes.c_int and args == [_lib._HANDLE, ctypes.POINTER(_lib.MtCem), ctypes.c_void_p, ctypes.c_int64,
                                            ctypes.c_int64]
    assert lib.mt_version() >= 420


def test_ctypes_cem_matches_c_layout(lib, tmp_path):
    from manytor_amd import _lib
    src = tmp_path / "cem_sz.c"
    offsets = ", ".join(f"offsetof(struct mt_cem,{f})" for f in FIELDS)
    fmt = " ".join(["%zu"] * (len(FIELDS) + 1))
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "manytor_hip.h"\n'
        f'int main(void){{printf("{fmt} %u %u\\n", sizeof(struct mt_cem), {offsets}, MT_CEM_AUTO_RESET, MT_CEM_KEEP_MEAN);'
        'return 0;}\n')
    exe = tmp_path / "cem_sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _lib.MtCem
    assert [name for name, _ in S._fields_] == list(FIELDS)
    assert c == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + [_lib.CEM_AUTO_RESET, _lib.CEM_KEEP_MEAN]


def test_null_handle_is_an_invalid_argument(lib):
    from manytor_amd import _lib
    s = _lib.MtCem()
    s.struct_size = ctypes.sizeof(_lib.MtCem)
    assert lib.mt_cem(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)
    assert lib.mt_cem(None, None) == _lib.MT_ERR_INVALID_ARG
    assert lib.mt_sample_plans(None, ctypes.byref(s), None, 0, 0) == _lib.MT_ERR_INVALID_ARG


def test_restated_noise_has_the_stated_moments():
    """Irwin-Hall of four uniform bytes, scaled: mean 0 +- 0.01, variance 1 +- 0.02 over 10^6 words, |z| <= 3.4506; the
    extremes are reached by the all-zero and all-ones words."""
    n = 250_000
    z = cem_ref.plan_noise(0x5EED, np.arange(n, dtype=np.uint64), 3, 1, 1, 4).ravel()      # 10^6 words of the plan stream
    assert z.size == 1_000_000 and z.dtype == np.float32
    z64 = z.astype(np.float64)
    print(f"[cem-noise] mean {z64.mean():+.5f} variance {z64.var():.5f} max |z| {np.abs(z64).max():.4f}")
    assert abs(z64.mean()) <= 0.01 and abs(z64.var() - 1.0) <= 0.02
    assert np.abs(z64).max() <= cem_ref.Z_MAX
    ends = cem_ref.noise(np.array([0, 0xFFFFFFFF, 0x7F80807F], dtype=np.uint32))           # byte sums 0, 1020, 510
    assert ends[0] == -ends[1] and abs(float(ends[1]) - 3.4506) < 1e-4 and ends[2] == 0
    # D = 7 draws its joints 4..6 from block 1, and block 0 is the same for any D
    z7 = cem_ref.plan_noise(0x5EED, np.arange(64, dtype=np.uint64), 3, 2, 3, 7)
    z4 = cem_ref.plan_noise(0x5EED, np.arange(64, dtype=np.uint64), 3, 2, 3, 4)
    np.testing.assert_array_equal(z7[:, :, :4], z4)
    assert (z7[:, :, 4:] != z4[:, :, :3]).mean() > 0.9


def test_restated_elite_rule_and_refit():
    returns = np.array([[1, 0, 2], [1, 0, 2], [0, 0, 3], [1, 0, 1]], dtype=np.float32)     # (C = 4, n = 3)
    np.testing.assert_array_equal(cem_ref.elite_mask(returns, 2), np.array([0b0011, 0b0011, 0b0101], dtype=np.uint64))
    np.testing.assert_array_equal(cem_ref.elite_mask(returns, 4), np.full(3, 0b1111, dtype=np.uint64))
    plans = np.arange(4 * 1 * 1 * 3, dtype=np.float32).reshape(4, 1, 1, 3)
    m, s = cem_ref.refit(plans, returns, 2, 0.0)
    np.testing.assert_array_equal(m[0, 0], [1.5, 2.5, 5.0])
    np.testing.assert_array_equal(s[0, 0], [1.5, 1.5, 3.0])
    np.testing.assert_array_equal(cem_ref.refit(plans, returns, 1, 0.25)[1], np.full((1, 1, 3), 0.25, dtype=np.float32))


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
    for call in (eng.cem, eng.sample_plans):
        kw = dict(candidates=4, elites=2) if call == eng.cem else dict(candidates=4)
        with pytest.raises(ValueError, match="CUDA float32"):
            call(host, host, **kw)                                          # host tensors are not read in place
        with pytest.raises(ValueError, match="CUDA float32"):
            call(np.zeros((T, d, n), dtype=np.float32), host, **kw)
        for c in (0, 65):
            with pytest.raises(ValueError, match="candidates"):
                call(host, host, **dict(kw, candidates=c))
        for lo, hi in ((float("nan"), 1.0), (-1.0, float("inf")), (2.0, 1.0), (-40000.0, 0.0)):
            with pytest.raises(ValueError, match="lo <= hi"):
                call(host, host, lo=lo, hi=hi, **kw)
    for e in (0, 5):
        with pytest.raises(ValueError, match="elites"):
            eng.cem(host, host, candidates=4, elites=e)
    with pytest.raises(ValueError, match="auto_reset"):
        eng.cem(host, host, candidates=4, elites=2, auto_reset=True)        # nothing to re-arm without a commit
    for bad in (float("nan"), -1.0, float("inf")):
        with pytest.raises(ValueError, match="sigma_min"):
            eng.cem(host, host, candidates=4, elites=2, sigma_min=bad)
    assert eng.version == 0
