"""CPU-only checks of mt_ik / mt_jacobian's host side -- the symbols are exported and prototyped, the ctypes mirror has the C
struct's layout, the flag values agree, and what the host can refuse without a handle is refused before a device is touched
(what needs the handle's shape is refused in tests/test_gpu_ik.py) -- and of the restatement the GPU tests hold the kernels
to (tests/ik_ref.py): its Jacobian against a central difference of the oracle's own fk, and its solver alone on the GPU
tests' inputs against the conditions those tests set."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ik_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("struct_size", "iters", "damping", "max_step_deg", "tol", "flags", "target", "target_ld", "start", "start_ld",
          "angles_out", "angles_ld", "residual_out", "iters_out", "index_out", "reserved")


@pytest.fixture(scope="module")
def lib():
    from manytor_amd import build, _lib
    build.build_library()            # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_calls_are_exported_and_prototyped(lib):
    from manytor_amd import _lib
    assert hasattr(lib, "mt_ik") and hasattr(lib, "mt_jacobian")
    assert _lib.PROTOTYPES["mt_ik"] == (ctypes.c_int, [_lib._HANDLE, ctypes.POINTER(_lib.MtIk)])
    res, args = _lib.PROTOTYPES["mt_jacobian"]
    assert res is ctypes.c_int and args == [_lib._HANDLE, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                            ctypes.c_void_p, ctypes.c_int64]
    assert lib.mt_version() >= 480


def test_ctypes_struct_and_flags_match_c(lib, tmp_path):
    from manytor_amd import _lib
    items = ["sizeof(struct mt_ik)"] + [f"offsetof(struct mt_ik,{f})" for f in FIELDS]
    items += ["(size_t)MT_IK_STAGE", "(size_t)MT_IK_WRAP", "(size_t)MT_IK_MAX_ITERS", "(size_t)MT_VERSION"]
    src = tmp_path / "ik_sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "manytor_hip.h"\n'
                   f'int main(void){{printf("{" ".join(["%zu"] * len(items))}\\n", {", ".join(items)});return 0;}}\n')
    exe = tmp_path / "ik_sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    c = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _lib.MtIk
    assert [name for name, _ in S._fields_] == list(FIELDS)
    want = [ctypes.sizeof(S)] + [getattr(S, f).offset for f in FIELDS]
    want += [_lib.IK_STAGE, _lib.IK_WRAP, _lib.IK_MAX_ITERS, lib.mt_version()]
    assert c == want
    assert (_lib.IK_STAGE, _lib.IK_WRAP) == (1, 2)


def _arg(_lib):
    s = _lib.MtIk()
    s.struct_size = ctypes.sizeof(s)
    s.iters, s.damping, s.max_step_deg, s.tol, s.flags = 16, 2.0, 30.0, 0.0, _lib.IK_WRAP
    s.target, s.target_ld, s.angles_out, s.angles_ld = 4096, 1 << 20, 8192, 1 << 20     # (never dereferenced: the handle is NULL)
    return s


def test_null_handle_is_invalid(lib):
    from manytor_amd import _lib
    assert lib.mt_ik(None, ctypes.byref(_arg(_lib))) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)
    assert lib.mt_ik(None, None) == _lib.MT_ERR_INVALID_ARG
    assert lib.mt_jacobian(None, None, 0, 4096, 1 << 20, None, 0) == _lib.MT_ERR_INVALID_ARG
    assert b"handle" in lib.mt_last_error(None)


@pytest.mark.parametrize("delta", [-8, 8, None])
def test_bad_struct_size_is_invalid(lib, delta):
    from manytor_amd import _lib
    s = _arg(_lib)
    s.struct_size = 0 if delta is None else ctypes.sizeof(s) + delta
    assert lib.mt_ik(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert b"struct_size" in lib.mt_last_error(None)


@pytest.mark.parametrize("field, value, word", [
    ("iters", 0, b"iters"), ("iters", 256, b"iters"), ("iters", -1, b"iters"),
    ("damping", 0.0, b"damping"), ("damping", float("nan"), b"damping"), ("damping", float("inf"), b"damping"),
    ("damping", -2.0, b"damping"), ("max_step_deg", 0.0, b"max_step_deg"), ("max_step_deg", float("nan"), b"max_step_deg"),
    ("tol", -1.0, b"tol"), ("tol", float("inf"), b"tol"), ("flags", 4, b"flags"), ("flags", 0x80000000, b"flags"),
    ("reserved", 1, b"reserved"), ("index_out", 4096, b"index_out"), ("angles_out", None, b"no output"),
])
def test_scalars_are_screened_ahead_of_the_handle(lib, field, value, word):
    from manytor_amd import _lib
    s = _arg(_lib)
    setattr(s, field, value)
    assert lib.mt_ik(None, ctypes.byref(s)) == _lib.MT_ERR_INVALID_ARG
    assert word in lib.mt_last_error(None)


# ---- ik_ref's own soundness ---------------------------------------------------------------------------------------------
def _oracle_point(q, table, f):
    from oracle import manytor_oracle as mo
    return np.array([mo.fk_matrix(f + 1, row, table)[0:3, 3] for row in q])


@pytest.mark.parametrize("arm", ["ref", "dh7", "rt6_f"])
def test_jacobian_agrees_with_a_central_difference_of_the_oracles_fk(arm):
    table, ee = ik_ref.arm_table(arm), ik_ref.ARMS[arm][2]
    dof = table.shape[0]
    f = ik_ref.resolve_frame(ee, dof)
    q = ik_ref.pose_case(arm, 24).astype(np.float64)
    J, p = ik_ref.jacobian(q, table, ee)
    assert np.abs(p - _oracle_point(q, table, f)).max() <= 1e-12
    h = 1e-4                                                     # degrees
    scale = np.abs(J).max()
    for j in range(dof):
        dq = np.zeros(dof)
        dq[j] = h
        fd = (_oracle_point(q + dq, table, f) - _oracle_point(q - dq, table, f)) / (2 * h)
        # the central difference's own error: h^2 / 6 * |p'''| <= (pi / 180)^2 h^2 / 6 * |J|, far below 1e-9 * |J|
        assert np.abs(J[:, :, j] - fd).max() <= 1e-8 * scale, (arm, j)
    assert scale > 0.1
    if arm == "rt6_f":
        assert f == dof - 2 and (J[:, :, f + 1:] == 0.0).all() and np.abs(J[:, :, f]).max() > 0
    assert ik_ref.jacobian(q, table, ee, per_degree=False)[0] == pytest.approx(J * 180.0 / np.pi, rel=1e-15)


def test_the_origin_row_is_refused():
    with pytest.raises(ValueError):
        ik_ref.resolve_frame(-4, 4)
    assert ik_ref.resolve_frame(-1, 4) == 3 and ik_ref.resolve_frame(-2, 6) == 4


def test_dh7_table_is_the_packages():
    from manytor_amd import engine
    assert np.array_equal(np.asarray(engine.DH7_TABLE), np.asarray(ik_ref.DH7_TABLE))
    assert np.array_equal(np.asarray(engine.REF_DH_TABLE), np.asarray(ik_ref.REF_TABLE))


@pytest.mark.parametrize("kind", ["zero", "random"])
@pytest.mark.parametrize("arm", ["ref", "dh7"])
def test_reference_alone_settles_the_gpu_tests_inputs(arm, kind):
    """The condition of test_gpu_ik's settled-outcome test, met by the restatement alone: at least 98 % of the envs are
    settled (fp64 box residual < 1e-3 after 16 and after 32 iterations)."""
    mask = ik_ref.settled_reference(arm, kind)
    print(f"ik_ref {arm} from {kind}: {100.0 * mask.mean():.2f} % settled")
    assert mask.shape == (ik_ref.SETTLED_N,) and mask.mean() >= ik_ref.SETTLED_SHARE


@pytest.mark.parametrize("arm", sorted(ik_ref.ARMS))
def test_reference_one_step_respects_the_cap_and_descends(arm):
    """One iteration on the GPU test's inputs: no joint moves more than max_step, some env hits the cap exactly, and the
    returned residual is the box residual of the returned angles."""
    x, q0 = ik_ref.step_case(arm, 200)
    table, ee = ik_ref.arm_table(arm), ik_ref.ARMS[arm][2]
    q, res, steps = ik_ref.ik(x, q0, table, ee, iters=1)
    move = np.abs(q - q0).max(axis=1)
    assert (move <= 30.0 * (1 + 1e-12)).all() and np.isclose(move.max(), 30.0) and (steps == 1).all()
    assert np.array_equal(res, ik_ref.box(x - ik_ref.position(q, table, ee)))


def test_early_stop_is_a_shorter_run():
    x, q0 = ik_ref.step_case("ref", 300)
    table = ik_ref.arm_table("ref")
    q, res, steps = ik_ref.ik(x, q0, table, iters=8, tol=1.0)
    assert steps.min() < 8 and steps.max() == 8
    assert (res[steps < 8] <= 1.0).all()
    for s in np.unique(steps):
        qs = q0 if s == 0 else ik_ref.ik(x, q0, table, iters=int(s))[0]
        assert np.array_equal(q[steps == s], qs[steps == s])


def test_unusable_input_and_missing_targets_hold_the_env():
    x, q0 = ik_ref.step_case("ref", 8)
    x, q0 = x.astype(np.float64), q0.astype(np.float64)
    x[1, 2], q0[2, 0], q0[3, 1], q0[4, 3] = np.nan, np.inf, 40000.0, -32768.0      # the last one is usable
    hold = np.zeros(8, dtype=bool)
    hold[5] = True
    q, res, steps = ik_ref.ik(x, q0, ik_ref.arm_table("ref"), iters=4, hold=hold)
    clean = ik_ref.ik(np.delete(x, [1, 2, 3, 5], axis=0), np.delete(q0, [1, 2, 3, 5], axis=0), ik_ref.arm_table("ref"), iters=4)
    for i in (1, 2, 3):
        assert np.array_equal(q[i], q0[i], equal_nan=True) and np.isnan(res[i]) and steps[i] == 0
    assert np.array_equal(q[5], q0[5]) and res[5] == 0 and steps[5] == 0
    keep = [0, 4, 6, 7]
    assert np.array_equal(q[keep], clean[0]) and np.array_equal(res[keep], clean[1]) and (steps[keep] == 4).all()


def test_wrap_maps_into_the_action_domain():
    q = np.array([-180.0, 179.999, 180.0, 540.0, -540.5, 0.0, 32767.5])
    w = ik_ref.wrap180(q)
    assert ((w >= -180.0) & (w < 180.0)).all()
    k = (q - w) / 360.0
    assert np.abs(k - np.rint(k)).max() < 1e-12


def test_nearest_takes_the_lowest_index_on_a_tie():
    table = ik_ref.arm_table("ref")
    q0 = np.zeros((3, 4))
    p = ik_ref.position(q0, table)[0]
    pts = np.tile(p, (3, 4, 1)) + np.array([[3.0, 0, 0], [0, 3.0, 0], [1.0, 0, 0], [0, 0, 1.0]])
    alive = np.array([[1, 1, 1, 1], [1, 1, 0, 0], [0, 0, 0, 0]])
    idx, d2 = ik_ref.nearest(pts, alive, q0, table)
    assert idx.tolist() == [2, 0, -1] and np.isinf(d2[1, 2:]).all()


def test_tolerance_constants_are_consistent():
    """The gates are 4 x what was measured on the GPU."""
    assert ik_ref.JAC_MEASURED > 0 and ik_ref.POS_MEASURED > 0 and ik_ref.STEP_MEASURED > 0
    assert ik_ref.JAC_TOL == 4.0 * ik_ref.JAC_MEASURED and ik_ref.POS_TOL == 4.0 * ik_ref.POS_MEASURED
    assert ik_ref.STEP_TOL == 4.0 * ik_ref.STEP_MEASURED
    assert ik_ref.SEQ_STEP_MEASURED > 0 and ik_ref.SEQ_STEP_TOL == 4.0 * ik_ref.SEQ_STEP_MEASURED
