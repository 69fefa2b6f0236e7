"""Seeded (prev, action) populations of STAGED steps over the whole accepted range of joint angles, +-32 768 degrees
(kernels.h: unusable_angle).  Shared by the oracle cross-check (test_oracle_golden.py, CPU) and the kernel parity tests
(test_gpu_staged_domain.py): the reference is vouched for on the very inputs the kernels are then held to.

Every array is fp32 -- what a policy hands to mt_step -- and, unless it says otherwise, fractional."""
import numpy as np

AMPLITUDES = (180, 720, 2048, 8192, 32768)
LIMIT = np.float32(32768.0)
BELOW = np.nextafter(LIMIT, np.float32(0))          # the largest float under the limit
ABOVE = np.nextafter(LIMIT, np.float32(np.inf))     # the first one that is refused


def wild(seed, n, dof, amplitude):
    """prev and action uniform in +-amplitude: routes of up to 2 * amplitude degrees per joint."""
    rng = np.random.RandomState(seed)
    prev = rng.uniform(-amplitude, amplitude, size=(n, dof)).astype(np.float32)
    action = rng.uniform(-amplitude, amplitude, size=(n, dof)).astype(np.float32)
    return prev, action


def local_turns(seed, n, dof):
    """A small pose (+-60) and a small move (+-30) of it, each shifted by whole turns, |m|, |m'| <= 90.  Half of the envs
    keep the turn count (m' = m: the route is the small move itself, seen from far out), a quarter change it by one turn on
    some joints, a quarter draw it afresh.  Unlike `wild`, whose routes nearly all sweep through the ground, this keeps
    both outcomes of the ground flag in play."""
    rng = np.random.RandomState(seed)
    small = rng.uniform(-60.0, 60.0, size=(n, dof))
    move = rng.uniform(-30.0, 30.0, size=(n, dof))
    m = rng.randint(-90, 91, size=(n, dof))
    kind = rng.randint(0, 4, size=n)                      # 0, 1: same turns   2: +-1 on some joints   3: random
    m2 = m.copy()
    one = rng.choice([-1, 0, 1], size=(n, dof))
    m2 = np.where((kind == 2)[:, None], np.clip(m + one, -90, 90), m2)
    m2 = np.where((kind == 3)[:, None], rng.randint(-90, 91, size=(n, dof)), m2)
    prev = (small + 360.0 * m).astype(np.float32)
    action = (small + move + 360.0 * m2).astype(np.float32)
    return prev, action


def edge_pairs(substeps):
    """(prev, action) scalars at the seams of the arithmetic."""
    f = np.float32
    tiny, sub = f(1e-45), f(1.1e-38)                      # the smallest denormal, and a large one
    pairs = [(LIMIT, -LIMIT), (-LIMIT, LIMIT), (LIMIT, LIMIT), (-LIMIT, -LIMIT), (f(0), LIMIT), (-LIMIT, f(0)),
             (BELOW, -BELOW), (f(0), BELOW), (-BELOW, f(17.25)), (BELOW, LIMIT),                 # (.., +-65 536 spans)
             (f(-0.0), tiny), (tiny, f(-0.0)), (-tiny, sub), (sub, -sub), (f(-0.0), f(0.0)), (f(90.5), -tiny)]
    # ties of the quadrant reduction x - 90 rint(x / 90): odd multiples of 45, whole; and the half degrees around them
    odd = 45.0 * (2 * np.arange(364) + 1)                 # 45, 135, ... 32 715
    for i, v in enumerate(odd):
        sgn = -1.0 if i % 2 else 1.0
        pairs.append((f(sgn * v), f(-sgn * odd[(7 * i + 3) % 364])))
        if i % 4 == 0:
            pairs.append((f(v + 0.5), f(v - 0.5)))
            pairs.append((f(-v - 0.5), f(22.5 * (2 * i + 1))))
    # increment of exactly 45 degrees per sub-step and the next float above it: the switch of sincos_increment
    span = 45.0 * (substeps - 1)
    for start in (0.0, 100.5, -span, 29000.25, -32768.0 + 11.0):
        s32 = f(start)
        pairs.append((s32, f(float(s32) + span)))
        pairs.append((s32, np.nextafter(f(float(s32) + span), f(np.inf))))
        pairs.append((f(float(s32) + span), s32))
    # an action that is the pose plus whole turns: the arm ends where it started
    for start, turns in ((12.625, 1), (-77.375, -1), (133.5, 5), (-3.75, -90), (0.0, 91), (211.0, -45)):
        pairs.append((f(start), f(start + 360.0 * turns)))
    return np.array(pairs, dtype=np.float32)


def edges(seed, n, dof, substeps):
    """One env per row of the edge list, the rest of the batch random (wild over the whole range, and local moves).
    Row layout: for every pair, one env with the pair on EVERY joint, then one env per joint with the pair on that joint
    alone and a fractional pose within +-180 on the others.  Returns prev, action, number of edge envs."""
    pairs = edge_pairs(substeps)
    rng = np.random.RandomState(seed)
    wp, wa = wild(seed + 1, n, dof, 32768)
    lp, la = local_turns(seed + 2, n, dof)
    half = rng.rand(n) < 0.5
    prev = np.where(half[:, None], wp, lp)
    action = np.where(half[:, None], wa, la)
    rows = len(pairs) * (dof + 1)
    assert rows <= n, (rows, n)
    r = 0
    for p, a in pairs:
        prev[r], action[r] = p, a
        r += 1
        for j in range(dof):
            prev[r] = rng.uniform(-180, 180, dof).astype(np.float32)
            action[r] = rng.uniform(-180, 180, dof).astype(np.float32)
            prev[r, j], action[r, j] = p, a
            r += 1
    return prev, action, rows


def make(population, seed, n, dof, substeps=25):
    """population: 'wild<A>', 'local' or 'edges'."""
    if population.startswith("wild"):
        return wild(seed, n, dof, int(population[4:]))
    if population == "local":
        return local_turns(seed, n, dof)
    if population == "edges":
        return edges(seed, n, dof, substeps)[:2]
    raise ValueError(population)


def fractional_offset_table():
    """A runtime 5-joint table whose theta offsets are not whole degrees (0.2 rad = 11.459..., -1.2 rad = -68.754...)."""
    rng = np.random.RandomState(77)
    off = np.array([0.2, -1.2, 0.0, 0.2, -1.2])
    return np.column_stack([rng.uniform(0, 9, 5), rng.choice([-np.pi / 2, 0.3, np.pi / 2], 5), rng.uniform(2, 12, 5), off]), 40.0
