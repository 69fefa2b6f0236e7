"""fp64 restatement of mt_jacobian / mt_ik (include/manytor_hip.h) -- TEST INFRASTRUCTURE ONLY.

The kernels (manytor_amd/csrc/kernels.h: ik_forward, jacobian_kernel, ik_kernel) are held to what is written here:

  chain      joint j at theta_j = radians(q_j) + off_j; one DH row = Rz(theta) Tz(d) Tx(a) Rx(alpha) (manytor.py:25-32)
  driven p   origin of row f = ee_frame mod D of joints_coordinates, f >= 1: the frame after f + 1 joints
  Jacobian   column j = z_j x (p - o_j) per radian for j <= f (z_j, o_j: Z axis and origin of the frame BEFORE joint j),
             exactly 0 for j > f; `jacobian` reports it per degree
  one step   e = x - p;  A = J J^T + lambda^2 I;  y = A^-1 e;  dq = degrees(J^T y);  m = max |dq|;  m > max_step: dq *= max_step / m
  early stop an env whose box residual max |e_a| is <= tol (tol > 0) before an iteration takes no further step
  held envs  non-finite target or unusable start angle (residual NaN); no alive target in nearest mode (residual 0)

Nothing here imports the product; arrays are env-major, (N, D) angles and (N, 3) points, as the oracle's are.
"""
import numpy as np

# ---- measured tolerances (the GPU tests assert them; tests/test_ik_host.py checks their arithmetic) -----------------------
# max |jacobian() - ik_ref.jacobian| per degree and max |position - fp64 chain| over every arm of tests/test_gpu_ik.py
# (static Ref4 / Dh7, runtime D = 2, 3, 4, 6, 8, ee_frame = -2) at whole-degree and fractional poses, measured on an MI355X.
JAC_MEASURED = 2.826e-07    # per degree (the 7-joint arm, n = 600)
JAC_TOL = 4.0 * JAC_MEASURED
POS_MEASURED = 1.411e-05    # length units (the 7-joint arm, n = 600)
POS_TOL = 4.0 * POS_MEASURED
# max |angles - ik_ref.ik| in degrees after ONE iteration (damping 2, max_step 30, whole-degree starts, reset()-law targets)
# over the same arms, measured on an MI355X.
STEP_MEASURED = 8.702e-04   # degrees (the reference arm through the runtime table, n = 200)
STEP_TOL = 4.0 * STEP_MEASURED
# max |angles - ik_ref.ik| in degrees, modulo 360, after FOUR iterations without early stop (damping 2, max_step 30, wrapped)
# from the fractional mid-episode poses of tests/test_gpu_call_sequences.py's oracle leg towards each env's nearest alive
# target: the reference arm, every regime of that test, over the unguarded sampled envs, measured on an MI355X.
# Far above four times STEP_MEASURED because the iteration itself amplifies: this fp64 restatement, run twice from the zero
# pose with the targets moved by 1e-5 (one fp32 rounding of the chain), differs from itself by up to 2.7e-2 degrees after
# three iterations (median 2.5e-5); the few envs near a singular pose set the maximum.
SEQ_STEP_MEASURED = 3.683e-02   # degrees (multi / per_step / chains / pop_*: the first ik of the sequence, about 3 000 envs)
SEQ_STEP_TOL = 4.0 * SEQ_STEP_MEASURED
# for orientation: a plain fp32 numpy restatement of the iteration differs from fp64 by at most this on 4 096 such cases
STEP_REF32_MEASURED = 1.8e-3
RESIDUAL_TOL = 1e-3         # residual_out against the fp64 residual of the RETURNED angles
SETTLED_TOL = 1e-3          # the guard band of the fused tests: a settled env's box residual, GPU angles through the fp64 chain
MAX_ANGLE = 32768.0         # unusable_angle's bound


def resolve_frame(ee_frame, dof):
    f = int(ee_frame) % dof
    if f == 0:
        raise ValueError("ee_frame resolves to the origin row, which no joint moves")
    return f


def frames(q_deg, table):
    """For poses (N, D): z (N, D, 3), o (N, D, 3) of the frames BEFORE each joint and p (N, D, 3), the origins after."""
    q = np.asarray(q_deg, dtype=np.float64)
    table = np.asarray(table, dtype=np.float64)
    n, dof = q.shape
    rot = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
    pos = np.zeros((n, 3))
    z, o, p = np.empty((n, dof, 3)), np.empty((n, dof, 3)), np.empty((n, dof, 3))
    for j in range(dof):
        a, alpha, d, off = table[j]
        z[:, j], o[:, j] = rot[:, :, 2], pos
        th = np.radians(q[:, j]) + off
        ct, st, ca, sa = np.cos(th), np.sin(th), np.cos(alpha), np.sin(alpha)
        m = np.zeros((n, 3, 3))
        m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = ct, -st * ca, st * sa
        m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = st, ct * ca, -ct * sa
        m[:, 2, 1], m[:, 2, 2] = sa, ca
        pos = pos + np.einsum("nij,nj->ni", rot, np.stack([a * ct, a * st, np.full(n, d)], axis=1))
        rot = np.einsum("nij,njk->nik", rot, m)
        p[:, j] = pos
    return z, o, p


def position(q_deg, table, ee_frame=-1):
    """The driven point (N, 3)."""
    f = resolve_frame(ee_frame, np.asarray(table).shape[0])
    return frames(q_deg, table)[2][:, f]


def jacobian(q_deg, table, ee_frame=-1, per_degree=True):
    """(J (N, 3, D), p (N, 3)): J[:, a, j] = d p_a / d q_j, per degree unless per_degree=False (then per radian)."""
    dof = np.asarray(table).shape[0]
    f = resolve_frame(ee_frame, dof)
    z, o, p = frames(q_deg, table)
    pt = p[:, f]
    J = np.zeros((pt.shape[0], 3, dof))
    for j in range(f + 1):
        J[:, :, j] = np.cross(z[:, j], pt - o[:, j])
    return (J * (np.pi / 180.0) if per_degree else J), pt


def box(e):
    return np.abs(e).max(axis=-1)


def usable(x, q0):
    """Envs whose input the solver accepts: finite target, start angles finite and within +-32768 degrees."""
    with np.errstate(invalid="ignore"):
        return np.isfinite(x).all(axis=1) & np.isfinite(q0).all(axis=1) & (np.abs(q0) <= MAX_ANGLE).all(axis=1)


def wrap180(q):
    return q - 360.0 * np.floor((q + 180.0) / 360.0)


def ik(x, q0, table, ee_frame=-1, iters=16, damping=2.0, max_step=30.0, tol=0.0, wrap=False, hold=None):
    """-> (angles (N, D), residual (N,), steps (N,) int32).  `hold`: envs to hold with residual 0 (nearest mode without an
    alive target); unusable input holds with residual NaN."""
    x = np.asarray(x, dtype=np.float64)
    q0 = np.asarray(q0, dtype=np.float64)
    n, dof = q0.shape
    ok = usable(x, q0)
    held = ~ok if hold is None else (~ok | np.asarray(hold, dtype=bool))
    q = np.where(held[:, None], 0.0, q0)
    xx = np.where(held[:, None], 0.0, x)
    frozen = held.copy()
    steps = np.zeros(n, dtype=np.int32)
    lam2 = float(damping) ** 2
    for _ in range(int(iters)):
        if frozen.all():
            break
        J, p = jacobian(q, table, ee_frame, per_degree=False)
        e = xx - p
        if tol > 0:
            frozen |= box(e) <= tol
        A = np.einsum("nij,nkj->nik", J, J) + lam2 * np.eye(3)
        y = np.linalg.solve(A, e[:, :, None])[:, :, 0]
        dq = np.degrees(np.einsum("nij,ni->nj", J, y))
        m = np.abs(dq).max(axis=1)
        scale = np.where(m > max_step, max_step / np.where(m > 0, m, 1.0), 1.0)
        go = ~frozen
        q[go] += (dq * scale[:, None])[go]
        steps[go] += 1
    if wrap:
        q = wrap180(q)
    res = box(xx - position(q, table, ee_frame))
    q = np.where(held[:, None], q0, q)
    res = np.where(held, 0.0, res)
    res = np.where(~ok, np.nan, res)
    return q, res, steps


def nearest(points, alive, q0, table, ee_frame=-1):
    """Nearest-target mode's choice: (index (N,) int32, -1 without an alive target; squared distances (N, K), inf where dead)."""
    points = np.asarray(points, dtype=np.float64)
    alive = np.asarray(alive).astype(bool)
    p = position(q0, table, ee_frame)
    d2 = ((points - p[:, None, :]) ** 2).sum(axis=-1)
    d2 = np.where(alive, d2, np.inf)
    idx = np.where(alive.any(axis=1), d2.argmin(axis=1), -1).astype(np.int32)   # (argmin: the lowest index wins a tie)
    return idx, d2


def draw_targets(rng, n, radius):
    """n points drawn as reset() draws them (manytor.py:229-239): uniform in the cube, kept inside the upper half ball."""
    out = np.empty((0, 3))
    while out.shape[0] < n:
        c = rng.uniform(-radius, radius, size=(2 * n + 16, 3))
        c = c[(c[:, 2] >= 0) & (np.sqrt((c ** 2).sum(axis=1)) <= radius)]
        out = np.concatenate([out, c])
    return out[:n].astype(np.float32)


def whole_degree_poses(rng, n, dof):
    return rng.randint(-180, 180, size=(n, dof)).astype(np.float32)


# ---- the arms and inputs of tests/test_gpu_ik.py (tests/test_ik_host.py runs the restatement alone on the same inputs) ----
_H = np.pi / 2
REF_TABLE = ((0.0, -_H, 4.3, 0.0), (0.0, _H, 0.0, 0.0), (0.0, -_H, 24.3, 0.0), (27.0, _H, 0.0, -_H))     # manytor.py:42-48
DH7_TABLE = ((0.0, -_H, 34.0, 0.0), (0.0, _H, 0.0, 0.0), (4.5, _H, 40.0, 0.0), (-4.5, -_H, 0.0, 0.0), (0.0, -_H, 40.0, 0.0),
             (8.8, _H, 0.0, -_H), (0.0, 0.0, 12.6, 0.0))
RT2_TABLE = ((0.0, -_H, 10.0, 0.0), (20.0, 0.0, 0.0, 0.0))
RT3_TABLE = ((0.0, -_H, 10.0, 0.0), (20.0, 0.0, 0.0, 0.3), (15.0, 0.0, 0.0, 0.0))
RT6_TABLE = ((0.0, -_H, 12.0, 0.0), (18.0, 0.0, 0.0, 0.0), (3.0, -_H, 0.0, 0.2), (0.0, _H, 16.0, 0.0), (5.0, -_H, 0.0, 0.0),
             (0.0, 0.0, 7.0, 0.0))
RT8_TABLE = ((0.0, -_H, 8.0, 0.0), (0.0, _H, 0.0, 0.0), (2.0, -_H, 14.0, 0.0), (0.0, _H, 0.0, 0.1), (0.0, -_H, 12.0, 0.0),
             (5.0, _H, 0.0, -_H), (0.0, -_H, 6.0, 0.0), (4.0, 0.0, 3.0, 0.0))
# name -> (table, radius the targets are drawn with, ee_frame, specialize)
ARMS = {
    "ref": (REF_TABLE, 51.3, -1, True),
    "dh7": (DH7_TABLE, 51.3, -1, True),
    "ref_rt": (REF_TABLE, 51.3, -1, False),
    "rt2": (RT2_TABLE, 25.0, -1, True),
    "rt3": (RT3_TABLE, 35.0, -1, True),
    "rt6": (RT6_TABLE, 40.0, -1, True),
    "rt8": (RT8_TABLE, 40.0, -1, True),
    "rt6_f": (RT6_TABLE, 35.0, -2, True),
}
SETTLED_N = 4096
SETTLED_SHARE = 0.98


def arm_table(arm):
    return np.asarray(ARMS[arm][0], dtype=np.float64)


def _rng(arm, n, salt):
    return np.random.RandomState(1000 * sorted(ARMS).index(arm) + 7 * n + salt)


def pose_case(arm, n):
    """Poses for the Jacobian test (n, D) float32: the first half whole degrees, the rest fractional, within +-180."""
    rng = _rng(arm, n, 1)
    dof = arm_table(arm).shape[0]
    q = whole_degree_poses(rng, n, dof)
    q[n // 2:] = rng.uniform(-180.0, 180.0, size=(n - n // 2, dof)).astype(np.float32)
    return q


def step_case(arm, n):
    """(targets (n, 3), starts (n, D)) float32: targets drawn as reset() draws them, random whole-degree starts."""
    rng = _rng(arm, n, 2)
    return draw_targets(rng, n, ARMS[arm][1]), whole_degree_poses(rng, n, arm_table(arm).shape[0])


def settled_case(arm, kind):
    """The settled-outcome inputs: SETTLED_N targets of radius 51.3, from the zero pose (kind "zero") or from random
    whole-degree poses ("random")."""
    rng = _rng(arm, SETTLED_N, 3 if kind == "zero" else 4)
    dof = arm_table(arm).shape[0]
    x = draw_targets(rng, SETTLED_N, 51.3)
    q0 = np.zeros((SETTLED_N, dof), dtype=np.float32) if kind == "zero" else whole_degree_poses(rng, SETTLED_N, dof)
    return x, q0


_SETTLED = {}


def settled_reference(arm, kind):
    """Which envs of settled_case are settled: the fp64 box residual is < SETTLED_TOL after 16 AND after 32 iterations
    (defaults: damping 2, max_step 30, no early stop).  Computed once."""
    if (arm, kind) not in _SETTLED:
        x, q0 = settled_case(arm, kind)
        table, ee = arm_table(arm), ARMS[arm][2]
        q16, r16, _ = ik(x, q0, table, ee, iters=16)
        _, r32, _ = ik(x, q16, table, ee, iters=16)               # (no early stop: 16 more iterations are iterations 17 .. 32)
        mask = (r16 < SETTLED_TOL) & (r32 < SETTLED_TOL)
        mask.setflags(write=False)
        _SETTLED[arm, kind] = mask
    return _SETTLED[arm, kind]
