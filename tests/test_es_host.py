"""CPU-only checks of the evolution-strategies calls' host side (mt_es_sample, mt_rollout_population, mt_es): the symbols
are exported and prototyped, the ctypes mirrors have the C structs' layout and constants, NULL arguments and a wrong
struct_size are refused before a device is touched, and the restatement the GPU test holds the kernels to
(tests/es_ref.py) is itself sound."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cem_ref
import es_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {
    "mt_es_sample": ("MtEsSample", ("struct_size", "n_members", "n_params", "theta", "pop", "pitch", "sigma", "draw", "seed",
                                    "reserved")),
    "mt_population": ("MtPopulation", ("struct_size", "n_steps", "n_members", "n_layers", "width", "hidden_act", "out_act", "pop",
                                       "pitch", "out_scale", "lo", "hi", "flags", "action_log", "act_ld", "obs_log", "obs_ld",
                                       "reward_log", "done_log", "log_ld", "return_out", "fitness_out", "seed", "reserved")),
    "mt_es": ("MtEs", ("struct_size", "shaping", "sigma", "lr", "draw", "flags", "theta", "grad_out", "best_out", "coeff_out",
                       "pop", "reserved")),
}
CONSTANTS = ("MT_ES_MAX_MEMBERS", "MT_ES_INPLACE", "MT_ES_UPDATE_ONLY", "MT_ES_SHAPE_RANK", "MT_ES_SHAPE_RAW")
ENTRY = {"mt_es_sample": "MtEsSample", "mt_rollout_population": "MtPopulation", "mt_es": "MtEs"}


@pytest.fixture(scope="module")
def lib():
    from manytor_amd import build, _lib
    build.build_library()            # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_es_calls_are_exported_and_prototyped(lib):
    from manytor_amd import _lib
    for name, struct in ENTRY.items():
        assert hasattr(lib, name)
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and args == [_lib._HANDLE, ctypes.POINTER(getattr(_lib, struct))]
    assert lib.mt_version() >= 450


def test_ctypes_structs_match_c_layout(lib, tmp_path):
    from manytor_amd import _lib
    items, fmt = [], []
    for cname, (_, fields) in STRUCTS.items():
        items.append(f"sizeof(struct {cname})")
        items += [f"offsetof(struct {cname},{f})" for f in fields]
        fmt += ["%zu"] * (len(fields) + 1)
    items += [f"(size_t){c}" for c in CONSTANTS]
    fmt += ["%zu"] * len(CONSTANTS)
    src = tmp_path / "es_sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "manytor_hip.h"\n'
                   f'int main(void){{printf("{" ".join(fmt)}\\n", {", ".join(items)});return 0;}}\n')
    exe = tmp_path / "es_sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for _, (pyname, fields) in STRUCTS.items():
        S = getattr(_lib, pyname)
        assert [name for name, _ in S._fields_] == list(fields)
        want += [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields]
    want += [_lib.ES_MAX_MEMBERS, _lib.ES_INPLACE, _lib.ES_UPDATE_ONLY, _lib.ES_SHAPE_RANK, _lib.ES_SHAPE_RAW]
    assert c == want


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_null_arguments_are_invalid(lib, name):
    from manytor_amd import _lib
    S = getattr(_lib, ENTRY[name])
    s = S()
    s.struct_size = ctypes.sizeof(S)
    fn = getattr(lib, name)
    assert fn(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)
    assert fn(None, None) == _lib.MT_ERR_INVALID_ARG


@pytest.mark.parametrize("name", sorted(ENTRY))
@pytest.mark.parametrize("delta", [-8, 8, None])
def test_bad_struct_size_is_invalid(lib, name, delta):
    """The struct is looked at ahead of the handle, so a block of another library version is named as such even here."""
    from manytor_amd import _lib
    S = getattr(_lib, ENTRY[name])
    s = S()
    s.struct_size = 0 if delta is None else ctypes.sizeof(S) + delta
    assert getattr(lib, name)(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"struct_size" in lib.mt_last_error(None)


# ---- es_ref's own soundness --------------------------------------------------------------------------------------
def test_noise_is_bounded_and_a_stream_of_its_own():
    z = es_ref.eps(0xABCDEF0123, 32, 3, 5003)
    assert z.dtype == np.float32 and z.shape == (32, 5003)
    assert float(np.abs(z).max()) <= cem_ref.Z_MAX
    assert abs(float(z.mean())) < 0.02 and abs(float(z.std()) - 1.0) < 0.02
    assert np.mean(z == es_ref.eps(0xABCDEF0123, 32, 4, 5003)) < 0.02          # another draw, another stream
    # pair p at parameter i has the plan stream's counter for env p but for the tag: the words differ
    plan = cem_ref.plan_noise(0xABCDEF0123, np.arange(32, dtype=np.uint64), 3, 1, 1, 4)[0, 0]          # (4, 32): block 0
    assert np.mean(plan.T == z[:, :4]) < 0.05
    # a shorter vector is a prefix
    np.testing.assert_array_equal(es_ref.eps(0xABCDEF0123, 32, 3, 17), z[:, :17])


def test_antithetic_rows_mirror_around_theta():
    theta = np.concatenate([np.zeros(9, np.float32), np.float32(0.25) * np.arange(-4, 5, dtype=np.float32)])      # exact at 0, at least
    M = 6
    e = es_ref.eps(11, M // 2, 0, theta.size)
    sigma = np.float32(2.0 ** -3)
    pop = es_ref.sample_population(theta, sigma, M, 0, 11)
    se = sigma * e
    exact = (((theta[None] + se).astype(np.float64) == theta[None].astype(np.float64) + se.astype(np.float64))
             & ((theta[None] - se).astype(np.float64) == theta[None].astype(np.float64) - se.astype(np.float64)))
    assert exact[:, :9].all() and exact.mean() > 0.5
    mid = (pop[0::2].astype(np.float64) + pop[1::2].astype(np.float64)) / 2
    np.testing.assert_array_equal(mid[exact], np.broadcast_to(theta.astype(np.float64), mid.shape)[exact])
    np.testing.assert_array_equal((pop[0::2] - theta[None])[exact], se[exact])


def test_mid_ranks_of_a_tied_vector_sum_to_m_m_minus_1():
    rng = np.random.RandomState(3)
    for M in (2, 6, 64):
        S = rng.randint(-3, 4, size=M)                                      # many ties
        c = es_ref.mid_ranks(S)
        assert int(c.sum()) == M * (M - 1)
        order = np.argsort(S, kind="stable")
        assert np.all(np.diff(c[order]) >= 0)                               # monotone in S
        assert np.all(c[S == S.max()] == c[es_ref.best(S)])
        assert es_ref.best(S) == int(np.flatnonzero(S == S.max())[0])
    np.testing.assert_array_equal(es_ref.mid_ranks([5, 5, 5, 5]), [3, 3, 3, 3])
    np.testing.assert_array_equal(es_ref.mid_ranks([1, 9, 1, 4]), [1, 6, 1, 4])


@pytest.mark.parametrize("shaping", ["raw", "rank"])
def test_constant_fitness_gives_a_zero_gradient(shaping):
    g, A = es_ref.gradient(np.full(8, -37, dtype=np.int64), 0.1, 256, 2, 99, 301, shaping)
    assert not A.any() and not g.any() and g.dtype == np.float32


def test_gradient_follows_the_better_half_of_a_pair():
    P, M = 64, 2
    b = es_ref.byte_sums(5, 1, 0, P)[0]
    g, A = es_ref.gradient(np.array([10, -10]), 0.5, 256, 0, 5, P, "raw")
    np.testing.assert_array_equal(A, 20 * b)
    want = (20 * b).astype(np.float32) * np.float32(float(cem_ref.KZ) / (M * 0.5 * 256))
    np.testing.assert_array_equal(g, want)
    np.testing.assert_array_equal(es_ref.apply(np.zeros(P, np.float32), g, 2.0), np.float32(2.0) * g)
    np.testing.assert_array_equal(es_ref.fitness([512, -256], 256), np.array([2.0, -1.0], dtype=np.float32))
