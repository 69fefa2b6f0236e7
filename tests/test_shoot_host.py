"""CPU-only checks of mt_shoot's host side: the symbol is exported, the ctypes mirror of struct mt_shoot has the C struct's
layout, and StepEngine.shoot refuses what it can refuse before it touches the library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("struct_size", "n_steps", "n_candidates", "commit_steps", "actions", "ld", "cand_stride", "returns_out", "ret_ld",
          "best_out", "best_return_out", "reward_log", "done_log", "log_ld", "return_out", "seed", "flags", "reserved")


@pytest.fixture(scope="module")
def lib():
    from manytor_amd import build, _lib
    build.build_library()            # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_shoot_is_exported_and_prototyped(lib):
    from manytor_amd import _lib
    assert hasattr(lib, "mt_shoot")
    res, args = _lib.PROTOTYPES["mt_shoot"]
    assert res is ctypes.c_int and args == [_lib._HANDLE, ctypes.POINTER(_lib.MtShoot)]
    assert lib.mt_version() >= 410


def test_ctypes_shoot_matches_c_layout(lib, tmp_path):
    from manytor_amd import _lib
    src = tmp_path / "shoot_sz.c"
    offsets = ", ".join(f"offsetof(struct mt_shoot,{f})" for f in FIELDS)
    fmt = " ".join(["%zu"] * (len(FIELDS) + 1))
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "manytor_hip.h"\n'
        f'int main(void){{printf("{fmt} %u\\n", sizeof(struct mt_shoot), {offsets}, MT_SHOOT_AUTO_RESET);return 0;}}\n')
    exe = tmp_path / "shoot_sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _lib.MtShoot
    assert [name for name, _ in S._fields_] == list(FIELDS)
    assert c == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + [_lib.SHOOT_AUTO_RESET]


def test_null_handle_is_an_invalid_argument(lib):
    from manytor_amd import _lib
    s = _lib.MtShoot()
    s.struct_size = ctypes.sizeof(_lib.MtShoot)
    assert lib.mt_shoot(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)
    assert lib.mt_shoot(None, None) == _lib.MT_ERR_INVALID_ARG


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched: {name}")


def test_python_front_end_refuses_before_it_touches_the_library(lib):
    """An engine object without a handle: every refusal below has to come from the argument checks alone."""
    from manytor_amd.engine import StepEngine
    n, d, T, c = 10, 4, 3, 2
    eng = object.__new__(StepEngine)
    eng.n_envs, eng.dof, eng.device, eng.version = n, d, 0, 0
    eng._lib = eng._h = _Untouchable()
    good = np.zeros((c, T, d, n), dtype=np.float32)
    with pytest.raises(ValueError, match="auto_reset"):
        eng.shoot(good, auto_reset=True)                                    # nothing to re-arm without a commit
    with pytest.raises(ValueError, match="auto_reset"):
        eng.shoot(good, commit=0, auto_reset=True)
    for bad in (np.zeros((T, d, n), dtype=np.float32),                      # a single tape
                np.zeros((c, T, d + 1, n), dtype=np.float32),
                np.zeros((c, T, d, n + 1), dtype=np.float32),
                np.zeros((c, T, n, d), dtype=np.float32)):                  # env-major data under the default layout
        with pytest.raises(ValueError, match="plans must be"):
            eng.shoot(bad)
    with pytest.raises(ValueError, match="plans must be"):
        eng.shoot(good, layout="env_major")
    with pytest.raises(ValueError, match="layout"):
        eng.shoot(good, layout="rows")
    # the 3-D form keeps its wording and its rules
    with pytest.raises(ValueError, match="actions must be"):
        eng._tape_tensor(good, "soa")
    assert eng.version == 0
