"""CPU-only checks of mt_rollout_tape's host side: the symbol is exported, the ctypes mirror of mt_tape has the C
struct's layout, and the entry point refuses a NULL handle before it touches a device."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ("struct_size", "n_steps", "actions", "ld", "reward_log", "done_log", "log_ld", "return_out", "seed", "flags",
          "reserved")


@pytest.fixture(scope="module")
def lib():
    from manytor_amd import build, _lib
    build.build_library()            # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_rollout_tape_is_exported_and_prototyped(lib):
    from manytor_amd import _lib
    assert hasattr(lib, "mt_rollout_tape")
    res, args = _lib.PROTOTYPES["mt_rollout_tape"]
    assert res is ctypes.c_int and args == [_lib._HANDLE, ctypes.POINTER(_lib.MtTape)]


def test_ctypes_tape_matches_c_layout(lib, tmp_path):
    from manytor_amd import _lib
    src = tmp_path / "tape_sz.c"
    offsets = ", ".join(f"offsetof(mt_tape,{f})" for f in FIELDS)
    fmt = " ".join(["%zu"] * (len(FIELDS) + 1))
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "manytor_hip.h"\n'
        f'int main(void){{printf("{fmt} %u %u\\n", sizeof(mt_tape), {offsets}, MT_TAPE_AUTO_RESET, MT_TAPE_DRY_RUN);return 0;}}\n')
    exe = tmp_path / "tape_sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _lib.MtTape
    assert [name for name, _ in S._fields_] == list(FIELDS)
    assert c == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in FIELDS] + [_lib.TAPE_AUTO_RESET, _lib.TAPE_DRY_RUN]


def test_null_handle_is_an_invalid_argument(lib):
    from manytor_amd import _lib
    t = _lib.MtTape()
    t.struct_size = ctypes.sizeof(_lib.MtTape)
    assert lib.mt_rollout_tape(None, ctypes.byref(t)) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)
    assert lib.mt_rollout_tape(None, None) == _lib.MT_ERR_INVALID_ARG
