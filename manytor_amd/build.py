"""Build libmanytor_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python -m manytor_amd.build            # build if sources are newer than the .so
    python -m manytor_amd.build --force
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
INCLUDE = os.path.join(os.path.dirname(PKG_DIR), "include")
LIB_PATH = os.path.join(PKG_DIR, "libmanytor_hip.so")
# one compiler process per source, side by side: engine.hip and actor_critic.hip hold the large kernel families
SOURCES = ["engine.hip", "actor_critic.hip", "comm.hip"]
DEPS = SOURCES + ["engine_internal.h", "step_args.h", "kernels.h", "table_dispatch.h", "mt_math.h", "philox.h"]


EXTRA_FLAGS = [
    # let x*0 and x+0 fold (static DH tables); staged actions are screened on their bit pattern (unusable_angle), so
    # no NaN/inf reaches the arithmetic of the step path
    "-fno-signed-zeros", "-ffinite-math-only",
    # gfx950 issues v_pk_*_f32 at half the rate of scalar VALU ops, so SLP-packing adjacent fp32 math only adds
    # register shuffles (measured: sub-step loop 66 -> 43 instructions, 72 -> 58 VGPRs without it)
    "-fno-slp-vectorize",
    # FMAs are written out in the source; no implicit contraction, so every kernel rounds a formula identically
    "-ffp-contract=off",
]


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm under /opt/rocm)")


def is_stale() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, d) for d in DEPS] + [os.path.join(INCLUDE, "manytor_hip.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force: bool = False, verbose: bool = False, extra_flags=()) -> str:
    if not force and not is_stale():
        return LIB_PATH
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fvisibility=hidden", "-I", INCLUDE, "-Wall",
             "-Wno-unused-function", *EXTRA_FLAGS, *extra_flags]
    with tempfile.TemporaryDirectory(prefix="manytor_build_") as tmp:
        jobs = []
        for src in SOURCES:
            obj = os.path.join(tmp, os.path.splitext(src)[0] + ".o")
            cmd = [_hipcc(), *flags, "-c", os.path.join(CSRC, src), "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            jobs.append((cmd, obj, subprocess.Popen(cmd)))
        failed = [cmd for cmd, _, proc in jobs if proc.wait() != 0]      # (every process is waited for)
        if failed:
            raise subprocess.CalledProcessError(1, failed[0])
        link = [_hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared", "-fvisibility=hidden", *[obj for _, obj, _ in jobs],
                "-o", LIB_PATH + ".tmp"]
        if verbose:
            print(" ".join(link), flush=True)
        subprocess.run(link, check=True)
    os.replace(LIB_PATH + ".tmp", LIB_PATH)
    return LIB_PATH


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
