"""The op alphabet, the sequence generator and the two followers of tests/test_gpu_call_sequences.py (importable without a
GPU: tests/test_call_sequences_host.py checks the generator and the oracle leg's guard-band cap on the CPU).

A sequence starts with reset_random(SEED, 0) and rollout(3, SEED, 0) and then runs every op of the alphabet twice, in an order
shuffled by a fixed seed: once as it comes and once with `rollout(2); reset_random(SEED, ep)` directly in front -- the rollout
so that the chains of a multi-chain handle are forked when the reset arrives (the comparison behind the previous op joined
them), the reset still deferred on the handles that defer when the op is entered.  Behind every op come sampled steps that
continue the step index with the same seed, alternating rollout(1..3, SEED, t) and step_random(SEED, t): the position in
which a stale pose record, target code or whole-degree flag would be used.  No env makes more than MAX_STEPS steps between
two full resets (the condition of the oracle leg's cap); where a stretch would, a reset_random and one sampled step are
put in ahead of the op (not directly in front of it: that is the other appearance).

The two kinds of appearance are shuffled on their own and dealt out in runs of BLOCK: a run without resets is one long
stretch in which envs finish, so the re-arming ops have somebody to re-arm and dead targets' codes get zeroed.

Step indices never restart: every sampled call of a sequence takes the index after the last one, whatever ran between.

Three ops take no argument of Data's: jacobian, ik and ik(stage)+step work on whatever the sequence left resident -- the
pose, and in nearest mode the targets and the alive mask -- so directly behind a reset_random they read the rows a deferred
reset has yet to write, and in a run of plain appearances rows whose targets were picked, zeroed by observe and re-armed.
ik(stage)+step is a reach controller's env-step: its angles are fractional, written to the action buffer by a kernel, and
the sampled steps behind it are the first to start from them.
"""
import collections

import numpy as np

import ik_ref

SEED = 0x5EC5
K = 7
TOL = 30.0          # a wide pickup box: targets get picked, and envs finish, within an episode
RING = 4
RADIUS = 51.3
T_TAPE = 3          # steps of a tape / a policy rollout / a plan (T <= 4)
C = 2               # candidates of shoot / cem / mppi
H = 2               # committed steps
WIDTH = 5           # the policies' one hidden layer
MEMBERS = 2
SIGMA_A = 5.0       # action noise of rollout_policy, degrees: fractional angles
SIGMA_P = 0.05      # parameter noise of es / sample_population
MAX_STEPS = 40
HEAD_STEPS = 3
SAVE_AHEAD = 3      # set_state restores the get_state() taken this many ops earlier
BLOCK = 12          # appearances without a reset in front come in runs of this many, then as many with one
IK_ITERS = 4        # ik: no early stop, every env with a target makes all of them
REACH_ITERS = 6     # ik(stage)+step: with the early stop at REACH_TOL, so lanes of a wave diverge and whole waves leave the loop
REACH_TOL = 1.0
REACH_FLOOR = 0.05  # ik(stage)+step is not vacuous: at least this share of the envs has a target to reach for and moves

# name -> env-steps the op makes
MOVING = collections.OrderedDict([
    ("step(host actions)", 1), ("set_actions(device)+step", 1), ("sample_actions+step", 1), ("step_host", 1), ("step_random", 1),
    ("env_step", 1), ("env_reset(points)", 0), ("env_reset(None)", 0), ("reset(points)", 0), ("reset_done", 0),
    ("rollout_fused(auto_reset=True)", 3), ("rollout_fused(auto_reset=False)", 3),
    ("rollout_actions", T_TAPE), ("rollout_actions(auto_reset=True)", T_TAPE),
    ("shoot(commit=H)", H), ("cem(commit=H)", H), ("mppi(commit=H)", H),
    ("rollout_policy", T_TAPE), ("rollout_policy(auto_reset=True)", T_TAPE),
    ("set(F_GOALS)", 0), ("set(F_POINTS)", 0), ("set(F_ALIVE)", 0), ("set_state", 0),
    ("ik(stage)+step", 1),
])
POPULATION = collections.OrderedDict([("rollout_population", T_TAPE), ("es", T_TAPE)])
NOTHING = ("rollout_actions(dry_run=True)", "shoot(commit=0)", "cem(commit=0)", "mppi(commit=0)", "sample_plans", "sample_population",
           "policy_eval", "policy_grad", "value_grad", "gae", "reward_to_go", "observe", "check_done", "bad_action_count", "get",
           "sync", "return_stats", "gather_begin+gather_wait", "gather_returns", "lap_begin+lap_end", "dispatch", "jacobian", "ik")
# the calls MT_ENTER_KEEP serves (they keep the host's record of MT_F_GOALS): the sampled steps behind them still re-derive
KEEPERS = ("sync", "get", "observe", "check_done", "bad_action_count", "lap_begin+lap_end", "jacobian", "ik")
LOG_MAKERS = ("rollout_policy", "rollout_policy(auto_reset=True)")
LOG_USERS = ("policy_eval", "policy_grad", "value_grad", "gae", "reward_to_go")
FULL_RESETS = ("reset(points)",)
SAMPLED_OPS = {"sample_actions+step": 1, "step_random": 1, "rollout_fused(auto_reset=True)": 3, "rollout_fused(auto_reset=False)": 3}
# no output of the call names the actions it committed: left out of the oracle leg's sequence, held by the twin leg
ORACLE_LEFT_OUT = ("es",)

FIELDS = ("F_GOALS", "F_ALIVE", "F_TOTAL_REWARD", "F_POINTS", "F_EPISODES", "F_LAST_RETURN", "F_OBS", "F_REWARD", "F_DONE",
          "F_EE", "F_DONE_BITS", "F_RETURN_RING")
# ... and, of handles created with debug_zmin=True, the minimum z the last step's ground test saw: the one output in which a
# table sine taken for a fractional start pose (a stale whole-degree flag) shows for EVERY env it happens to, not only for the
# few whose ground flag it flips
SNAP_FIELDS = FIELDS + ("F_ZMIN",)

# pre / trail items: ("save_state",), ("reset_random", ep), ("rollout", steps, t0), ("step_random", t0)
Group = collections.namedtuple("Group", "op with_reset pre trail t ep")


def population_ok(n):
    return n % MEMBERS == 0 and (n // MEMBERS) % 256 == 0


def alphabet(n, oracle=False):
    ops = list(MOVING) + (list(POPULATION) if population_ok(n) else []) + list(NOTHING)
    return [o for o in ops if not (oracle and o in ORACLE_LEFT_OUT)]


def op_steps(op):
    return MOVING.get(op, POPULATION.get(op, 0))


def generate(shuffle, n, oracle=False):
    """-> (head, groups): head the items every sequence starts with, groups one Group per appearance of an op."""
    ops = alphabet(n, oracle)
    # both appearances shuffled on their own, then dealt out in runs of BLOCK: a run of plain appearances is one long
    # stretch without a full reset, in which envs finish (and the re-arming ops have somebody to re-arm)
    rs = np.random.RandomState(1000 + shuffle)
    plain = [(ops[i], False) for i in rs.permutation(len(ops))]
    fresh = [(ops[i], True) for i in rs.permutation(len(ops))]
    entries = []
    for b in range(0, len(ops), BLOCK):
        entries += plain[b:b + BLOCK] + fresh[b:b + BLOCK]
    # the logs of a policy rollout exist before the first call that reads them
    maker = min(i for i, (o, _) in enumerate(entries) if o in LOG_MAKERS)
    user = min(i for i, (o, _) in enumerate(entries) if o in LOG_USERS)
    if user < maker:
        entries[user], entries[maker] = entries[maker], entries[user]
    save_at = {max(0, i - SAVE_AHEAD) for i, (o, _) in enumerate(entries) if o == "set_state"}

    head = [("reset_random", 0), ("rollout", HEAD_STEPS, 0)]
    t, ep, age, saved_age = HEAD_STEPS, 0, HEAD_STEPS, None
    groups = []
    for i, (op, with_reset) in enumerate(entries):
        pre, trail = [], []

        def sampled(into, steps):
            nonlocal t, age
            into.append(("rollout", steps, t) if steps else ("step_random", t))
            t += max(1, steps)
            age += max(1, steps)

        def refresh():   # a full reset that is NOT directly in front of the op
            nonlocal ep, age
            ep += 1
            pre.append(("reset_random", ep))
            age = 0
            sampled(pre, 1)

        tail = 0 if i % 2 else 1 + (i // 2) % 3          # rollout(1..3) and step_random (0) in turn
        cost = op_steps(op) + max(1, tail)
        if i in save_at:
            if age + cost + 3 > MAX_STEPS - 3:           # the state restored later is this old again, plus that op's tail
                refresh()
            pre.append(("save_state",))
            saved_age = age
        if with_reset:
            if age + 2 > MAX_STEPS:
                refresh()
            sampled(pre, 2)
            ep += 1
            pre.append(("reset_random", ep))
            age = 0
        elif op not in FULL_RESETS and (saved_age if op == "set_state" else age) + cost > MAX_STEPS:
            refresh()                                    # (set_state: the saved state was taken young enough, above)
        t_op = t
        if op in SAMPLED_OPS:
            t += SAMPLED_OPS[op]
        if op in FULL_RESETS:
            age = 0
        if op == "set_state":
            age = saved_age
        age += op_steps(op)
        sampled(trail, tail)
        groups.append(Group(op, with_reset, tuple(pre), tuple(trail), t_op, ep))
    return head, groups


def stretches(head, groups):
    """The env-steps of every stretch between two full resets, walked over the sequence as written (independent of the
    generator's own bookkeeping); set_state continues the stretch its state was saved in."""
    out, age, saved = [], 0, 0

    def item(it):
        nonlocal age, saved
        if it[0] == "reset_random":
            out.append(age)
            age = 0
        elif it[0] == "rollout":
            age += it[1]
        elif it[0] == "step_random":
            age += 1
        elif it[0] == "save_state":
            saved = age
    for it in head:
        item(it)
    for g in groups:
        for it in g.pre:
            item(it)
        if g.op in FULL_RESETS:
            out.append(age)
            age = 0
        if g.op == "set_state":
            out.append(age)
            age = saved
        age += op_steps(g.op)
        for it in g.trail:
            item(it)
    out.append(age)
    return out


def sample_of(n, span):
    """The envs the oracle plays: the first and the last 512, 512 on each side of the chain boundary, a stride of 37 over the
    rest, thinned to about 4 000 in all."""
    rest = np.arange(0, n, 37)
    if len(rest) > 1950:
        rest = rest[::-(-len(rest) // 1950)]
    parts = [np.arange(min(512, n)), np.arange(max(0, span - 512), min(n, span + 512)), np.arange(max(0, n - 512), n), rest,
             np.array(single_envs(n, span))]
    return np.unique(np.concatenate(parts))


def single_envs(n, span):
    """One env in the first block, one on each side of the chain boundary (the middle of a one-chain batch), one in the
    ragged last block."""
    mid = span if span < n else (n // 2)
    return [3, mid - 1, mid, n - 2]


class Data:
    """The fixed arguments of the ops for a batch of n envs, host arrays (env axis first unless the name says otherwise)."""

    def __init__(self, n, span):
        rng = np.random.default_rng(11)
        self.n, self.span = n, span
        self.envs = single_envs(n, span)

        def angles(*lead):
            a = rng.integers(-180, 180, size=lead + (n, 4)).astype(np.float32)
            a[..., 1::2, :] += rng.uniform(-0.5, 0.5, size=a[..., 1::2, :].shape).astype(np.float32)   # whole and fractional degrees
            return a
        self.acts = [angles() for _ in range(3)]                      # step(host), set_actions(device), step_host
        for i, a in enumerate(self.acts):
            a[i::5, 1] = np.nan                                       # unusable: those envs hold their pose
        self.poses = angles()                                         # set(F_GOALS)
        self.tapes = [angles(T_TAPE), angles(T_TAPE)]                 # rollout_actions: (T, N, D)
        self.tapes[0][1, 2::7, 3] = np.nan
        self.plans = np.ascontiguousarray(angles(C, T_TAPE).transpose(0, 1, 3, 2))   # shoot: (C, T, D, N)
        self.mean = np.ascontiguousarray(angles(T_TAPE).transpose(0, 2, 1))          # cem / mppi: (T, D, N)
        self.sigma = np.full_like(self.mean, 20.0)

        def targets(*lead):
            p = rng.uniform(-40.0, 40.0, size=lead + (K, 3)).astype(np.float32)
            p[..., 2] = np.abs(p[..., 2])
            return p
        self.pts_set, self.pts_reset, self.pts_env = targets(n), targets(n), targets()
        self.alive = (rng.uniform(size=(n, K)) < 0.8).astype(np.uint8)
        self.env_acts = angles()[:4].copy()
        self.env_acts[1::2] += np.float32(0.25)
        n_in = 3 * K
        self.policy = [((rng.standard_normal((WIDTH, n_in)) * 0.02).astype(np.float32), (rng.standard_normal(WIDTH) * 0.1).astype(np.float32)),
                       ((rng.standard_normal((4, WIDTH)) * 0.8).astype(np.float32), (rng.standard_normal(4) * 0.1).astype(np.float32))]
        self.value = [((rng.standard_normal((WIDTH, n_in)) * 0.02).astype(np.float32), (rng.standard_normal(WIDTH) * 0.1).astype(np.float32)),
                      ((rng.standard_normal((1, WIDTH)) * 0.5).astype(np.float32), (rng.standard_normal(1) * 0.1).astype(np.float32))]
        self.theta = np.concatenate([t.ravel() for pair in self.policy for t in pair]).astype(np.float32)
        self.pop = np.stack([self.theta + np.float32(0.03) * rng.standard_normal(self.theta.shape).astype(np.float32)
                             for _ in range(MEMBERS)]).astype(np.float32)
        self._dev = None

    def dev(self, device):
        """The device copies (made once, read-only: shared by the handle under test and its twin)."""
        if self._dev is None:
            import torch
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            self._dev = dict(acts=to(self.acts[1]), tapes=[to(t) for t in self.tapes], plans=to(self.plans), mean=to(self.mean),
                             sigma=to(self.sigma), policy=[(to(w), to(b)) for w, b in self.policy],
                             value=[(to(w), to(b)) for w, b in self.value], theta=to(self.theta), pop=to(self.pop))
        return self._dev


# ------------------------------------------------------------------------------------------------------------------------
# the engine's side: one call sequence on one handle
# ------------------------------------------------------------------------------------------------------------------------
class Runner:
    def __init__(self, m, eng, data):
        import torch
        self.m, self.e, self.d = m, eng, data
        self.D = data.dev(torch.device("cuda", eng.device))
        self.logs = None
        self.saved = None

    def item(self, it):
        e = self.e
        if it[0] == "reset_random":
            e.reset_random(SEED, it[1])
        elif it[0] == "rollout":
            e.rollout(it[1], SEED, it[2])
        elif it[0] == "step_random":
            e.step_random(SEED, it[1])
        elif it[0] == "save_state":
            self.saved = e.get_state()
        else:
            raise KeyError(it)

    def field(self, name):
        """One field as an env-major device tensor: mt_get into device memory -- what get() does, without the host copy that
        would dominate a sequence at 300 000 envs.  (uint32 / uint64 fields come as the signed type of their width.)"""
        import ctypes
        import torch
        e = self.e
        shape, dt = e._shape_dtype(getattr(self.m.lib, name))
        tdt = {np.float32: torch.float32, np.int32: torch.int32, np.uint8: torch.uint8, np.uint32: torch.int32,
               np.uint64: torch.int64}[dt]
        t = torch.empty(shape, dtype=tdt, device=torch.device("cuda", e.device))
        e._call(e._lib.mt_get, getattr(self.m.lib, name), ctypes.c_void_p(t.data_ptr()), ctypes.c_int64(t.numel() * t.element_size()), 1)
        return t

    def snapshot(self):
        """The twelve fields and F_ZMIN, complete when this returns."""
        import torch
        torch.cuda.current_stream(self.e.device).synchronize()    # (nothing of torch's still reads a block this reuses)
        snap = {f: self.field(f) for f in SNAP_FIELDS}
        self.e.sync()
        return snap

    def rows(self, names, idx):
        """The rows `idx` (a device index tensor) of some fields, as host arrays."""
        import torch
        torch.cuda.current_stream(self.e.device).synchronize()
        full = {f: self.field(f) for f in names}
        self.e.sync()
        return to_host({f: t.index_select(0, idx) for f, t in full.items()})

    def op(self, g):
        """Runs the op; -> {name: output} (device tensors, host arrays or numbers) of everything the call returned."""
        import torch
        e, d, D, lib = self.e, self.d, self.D, self.m.lib
        op, out = g.op, {}
        kw_log = dict(log=True, returns=True)
        if op == "step(host actions)":
            e.step(d.acts[0])
        elif op == "set_actions(device)+step":
            e.set_actions(D["acts"])
            e.step()
        elif op == "sample_actions+step":
            e.sample_actions(SEED, g.t)
            e.step()
        elif op == "step_host":
            out = dict(zip(("obs", "reward", "done"), e.step_host(d.acts[2])))
        elif op == "step_random":
            e.step_random(SEED, g.t)
        elif op == "env_step":
            for i, env in enumerate(d.envs):
                o, r, dn = e.env_step(env, d.env_acts[i])
                out.update({f"obs{i}": o, f"reward{i}": r, f"done{i}": dn})
        elif op == "env_reset(points)":
            for env in d.envs:
                e.env_reset(env, d.pts_env, SEED, g.ep)
        elif op == "env_reset(None)":
            for env in d.envs:
                e.env_reset(env, None, SEED, g.ep + 50)
        elif op == "reset(points)":
            e.reset(d.pts_reset)
        elif op == "reset_done":
            e.reset_done(SEED)
        elif op.startswith("rollout_fused"):
            e.rollout_fused(3, SEED, g.t, auto_reset="True" in op)
        elif op == "rollout_actions":
            out = e.rollout_actions(D["tapes"][0], **kw_log)
        elif op == "rollout_actions(auto_reset=True)":
            out = e.rollout_actions(D["tapes"][1], auto_reset=True, seed=SEED, **kw_log)
        elif op == "rollout_actions(dry_run=True)":
            out = e.rollout_actions(D["tapes"][0], dry_run=True, **kw_log)
        elif op.startswith("shoot"):
            out = e.shoot(D["plans"], commit=H if "H" in op else 0, all_returns=True, **(kw_log if "H" in op else {}))
        elif op.startswith("cem"):
            out = e.cem(D["mean"], D["sigma"], candidates=C, elites=1, draw=g.t, seed=SEED, commit=H if "H" in op else 0,
                        all_returns=True, **(kw_log if "H" in op else {}))
        elif op.startswith("mppi"):
            out = e.mppi(D["mean"], D["sigma"], candidates=C, temperature=1.0, draw=g.t, seed=SEED, commit=H if "H" in op else 0,
                         all_returns=True, **(kw_log if "H" in op else {}))
        elif op.startswith("rollout_policy"):
            out = e.rollout_policy(D["policy"], T_TAPE, sigma=SIGMA_A, draw=g.t, seed=SEED, auto_reset="True" in op, actions=True,
                                   observations=True, **kw_log)
            self.logs = out
        elif op == "set(F_GOALS)":
            e.set(lib.F_GOALS, d.poses)
        elif op == "set(F_POINTS)":
            e.set(lib.F_POINTS, d.pts_set)
        elif op == "set(F_ALIVE)":
            e.set(lib.F_ALIVE, d.alive)
        elif op == "set_state":
            e.set_state(self.saved)
        elif op == "rollout_population":
            out = e.rollout_population(D["pop"], T_TAPE, widths=(WIDTH,), seed=SEED, actions=True, **kw_log)
        elif op == "es":
            out = e.es(D["theta"], SIGMA_P, members=MEMBERS, steps=T_TAPE, widths=(WIDTH,), draw=g.t, seed=SEED, log=True)
        elif op == "sample_plans":
            out = {"plans": e.sample_plans(D["mean"], D["sigma"], candidates=C, draw=g.t, seed=SEED)}
        elif op == "sample_population":
            out = {"population": e.sample_population(D["theta"], SIGMA_P, members=MEMBERS, draw=g.t, seed=SEED)}
        elif op in LOG_USERS:
            lg = self.logs
            coef = lg["reward"].to(torch.float32)
            if op == "policy_eval":
                out = e.policy_eval(D["policy"], lg["observations"], actions=lg["actions"], sigma=SIGMA_A)
            elif op == "policy_grad":
                out = dict(zip(("grad", "loss"), e.policy_grad(D["policy"], lg["observations"], lg["actions"], coef, sigma=SIGMA_A,
                                                               loss=True)))
            elif op == "value_grad":
                out = dict(zip(("grad", "loss"), e.value_grad(D["value"], lg["observations"], coef, loss=True)))
            elif op == "gae":
                out = e.gae(lg["reward"], lg["done"], e.values(D["value"], lg["observations"]).contiguous(), weights=True)
            else:
                out = {"reward_to_go": e.reward_to_go(lg["reward"], lg["done"], gamma=0.9)}
        elif op == "observe":
            e.observe()
        elif op == "check_done":
            e.check_done()
        elif op == "bad_action_count":
            out = {"count": e.bad_action_count()}
        elif op == "get":
            out = {f: e.get(getattr(lib, f)) for f in FIELDS + ("F_ACTIONS", "F_JOINTS")}
        elif op == "sync":
            e.sync()
        elif op == "return_stats":
            out = e.return_stats()
        elif op == "gather_begin+gather_wait":
            out = {"gathered": e.gather_begin()}
            e.gather_wait(host=True)
        elif op == "gather_returns":
            out = {"gathered": e.gather_returns()}
            e.sync()
        elif op == "lap_begin+lap_end":
            e.lap_begin()
            e.lap_end()
        elif op == "dispatch":
            e.dispatch()
        elif op == "jacobian":
            out = dict(zip(("jacobian", "position"), e.jacobian(position=True)))
        elif op == "ik":
            out = e.ik(iters=IK_ITERS, tol=0.0, steps=True)
        elif op == "ik(stage)+step":
            out = e.ik(stage=True, iters=REACH_ITERS, tol=REACH_TOL, steps=True)
            e.step()
        else:
            raise KeyError(op)
        return dict(out or {})


def to_host(snap):
    """A snapshot's fields as the arrays get() returns."""
    unsigned = {np.dtype(np.int32): np.uint32, np.dtype(np.int64): np.uint64}
    out = {}
    for f, t in snap.items():
        a = t.cpu().numpy()
        out[f] = a.view(unsigned[a.dtype]) if f in ("F_EPISODES", "F_DONE_BITS") else a
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the oracle's side: the same sequence on oracle.manytor_oracle.BatchOracle, fp64, for a sample of the envs
# ------------------------------------------------------------------------------------------------------------------------
class OracleFollower:
    """BatchOracle plus what the engine adds to the reference: per-env episode counters, the re-arm of finished envs (new
    targets keyed by (seed, env, episode)), the done byte's three states, actions that are held, and the guard band: an env
    that came within GUARD of a ground or pickup threshold is out of the exact comparisons until the next full reset."""

    def __init__(self, sample, data, guard):
        from oracle import manytor_oracle as mo
        from oracle import philox_ref as px
        self.mo, self.px, self.GUARD = mo, px, guard
        self.sample = np.asarray(sample)
        self.ids = self.sample.astype(np.uint64)
        self.d = data
        m_ = len(self.sample)
        self.ora = mo.BatchOracle(m_, K, pickup_tol=TOL)
        self.episodes = np.zeros(m_, dtype=np.int64)
        self.done_state = np.zeros(m_, dtype=np.uint8)     # 1 finished, 2 finished and re-armed in the same call
        self.guarded = np.zeros(m_, dtype=bool)
        self.saved = None
        self.rearmed = 0                                   # envs re-armed so far (reset_done, auto_reset)
        self.last = dict(obs=np.zeros((m_, 3 * K)), rew=np.zeros(m_, dtype=np.int64), done=np.zeros(m_, dtype=bool),
                         jc=self.ora.joints_coordinates.copy(), pre_alive=np.ones((m_, K), dtype=bool),
                         points=self.ora.points.copy(), zmin=np.zeros(m_))
        self.log = []                                      # (reward, done) of every step of the last op
        pos = {int(e): i for i, e in enumerate(self.sample)}
        self.single = np.array([pos[e] for e in data.envs])   # the single-env ops' envs are part of every sample

    # ---- resets ----
    def _posed(self):
        o = self.ora
        o.joints_coordinates = self.mo.batch_joints_coordinates(o.goals, o.table, o.dtype)

    def full_reset(self, points, episode):
        self.ora.reset(np.asarray(points, dtype=np.float64))
        self.episodes[:] = episode
        self.done_state[:] = 0
        self.guarded[:] = False

    def reset_random(self, ep):
        self.full_reset(self.px.sample_targets(SEED, self.ids, ep, K, RADIUS), ep)

    def rearm(self, idx, byte):
        o = self.ora
        if len(idx):
            self.rearmed += len(idx)
            self.episodes[idx] += 1
            o.goals[idx] = 0.0
            o.total_reward[idx] = 0.0
            o.alives[idx] = True
            o.points[idx] = self.px.sample_targets(SEED, self.ids[idx], self.episodes[idx], K, RADIUS).astype(np.float64)
            self._posed()
        self.done_state[idx] = byte

    # ---- steps ----
    def step(self, actions, auto_reset=False):
        o = self.ora
        a = np.array(actions, dtype=np.float64).reshape(o.n, o.dof)
        with np.errstate(invalid="ignore"):
            bad = ~(np.abs(a) <= 32768.0).all(axis=1)      # NaN, infinite or beyond the accepted magnitude: the pose is held
        a[bad] = o.goals[bad]
        pre_alive = o.alives.copy()
        obs, rew, done = o.step(a)
        pm = np.where(pre_alive, o.pickup_margin, np.inf).min(axis=1)
        self.guarded |= (o.ground_margin < self.GUARD) | (pm < self.GUARD)
        self.last = dict(obs=obs, rew=rew, done=done, jc=o.joints_coordinates.copy(), pre_alive=pre_alive, points=o.points.copy(),
                         zmin=o.zmin.copy())
        self.log.append((rew.copy(), done.copy()))
        self.done_state = done.astype(np.uint8)
        if auto_reset:
            self.rearm(np.flatnonzero(done), 2)

    def sampled(self, t, steps=1):
        for s in range(steps):
            self.step(self.px.sample_actions(SEED, self.ids, t + s, 4))

    def env_step(self, idx, actions):
        """One step of the envs `idx` alone: on a BatchOracle of their own, copied out of and back into the batch."""
        o = self.ora
        sub = self.mo.BatchOracle(len(idx), K, pickup_tol=TOL)
        sub.goals, sub.points, sub.alives = o.goals[idx].copy(), o.points[idx].copy(), o.alives[idx].copy()
        sub.total_reward = o.total_reward[idx].copy()
        a = np.array(actions, dtype=np.float64)
        pre_alive = sub.alives.copy()
        obs, rew, done = sub.step(a)
        pm = np.where(pre_alive, sub.pickup_margin, np.inf).min(axis=1)
        self.guarded[idx] |= (sub.ground_margin < self.GUARD) | (pm < self.GUARD)
        o.goals[idx], o.points[idx], o.alives[idx], o.total_reward[idx] = sub.goals, sub.points, sub.alives, sub.total_reward
        self._posed()
        for key, v in (("obs", obs), ("rew", rew), ("done", done), ("jc", sub.joints_coordinates), ("pre_alive", pre_alive),
                       ("points", sub.points), ("zmin", sub.zmin)):
            self.last[key][idx] = v
        self.done_state[idx] = done.astype(np.uint8)

    def reach(self, iters, tol):
        """What ik(iters=, tol=) in nearest mode from the resident pose returns, by ik_ref on the oracle's own state:
        (angles (m, D), residual, steps, index), wrapped into [-180, 180); an env without an alive target is held."""
        o = self.ora
        index, _ = ik_ref.nearest(o.points, o.alives, o.goals, o.table, o.ee_frame)
        x = o.points[np.arange(o.n), np.maximum(index, 0)]
        angles, residual, steps = ik_ref.ik(x, o.goals, o.table, o.ee_frame, iters=iters, tol=tol, wrap=True, hold=index < 0)
        return angles, residual, steps, index

    # ---- the sequence ----
    def item(self, it):
        if it[0] == "reset_random":
            self.reset_random(it[1])
        elif it[0] == "rollout":
            self.sampled(it[2], it[1])
        elif it[0] == "step_random":
            self.sampled(it[1])
        elif it[0] == "save_state":
            o = self.ora
            self.saved = dict(goals=o.goals.copy(), points=o.points.copy(), alives=o.alives.copy(), total=o.total_reward.copy(),
                              episodes=self.episodes.copy(), done_state=self.done_state.copy(), guarded=self.guarded.copy())

    def op(self, g, committed):
        """The op on the oracle.  committed(name) -> (T, m, D): the actions of the sampled envs the engine's call committed,
        for the ops whose actions the library chooses (planners, policies)."""
        o, d, s = self.ora, self.d, self.sample
        op = g.op
        self.log = []
        if op == "step(host actions)":
            self.step(d.acts[0][s])
        elif op == "set_actions(device)+step":
            self.step(d.acts[1][s])
        elif op == "step_host":
            self.step(d.acts[2][s])
        elif op in ("sample_actions+step", "step_random"):
            self.sampled(g.t)
        elif op == "env_step":
            self.env_step(self.single, d.env_acts)
        elif op.startswith("env_reset"):
            i = self.single
            o.goals[i], o.total_reward[i], o.alives[i] = 0.0, 0.0, True
            if op == "env_reset(points)":
                o.points[i], self.episodes[i] = d.pts_env.astype(np.float64), g.ep
            else:
                self.episodes[i] = g.ep + 50
                o.points[i] = self.px.sample_targets(SEED, self.ids[i], self.episodes[i], K, RADIUS).astype(np.float64)
            self.done_state[i] = 0
            self._posed()
        elif op == "reset(points)":
            self.full_reset(d.pts_reset[s], 0)
        elif op == "reset_done":
            self.rearm(np.flatnonzero(self.done_state == 1), 0)
            self.done_state[:] = 0
        elif op.startswith("rollout_fused"):
            for q in range(3):
                self.step(self.px.sample_actions(SEED, self.ids, g.t + q, 4), auto_reset="True" in op)
        elif op in ("rollout_actions", "rollout_actions(auto_reset=True)"):
            tape = d.tapes[1 if "True" in op else 0]
            for q in range(T_TAPE):
                self.step(tape[q][s], auto_reset="True" in op)
        elif op in ("shoot(commit=H)", "cem(commit=H)", "mppi(commit=H)", "rollout_policy", "rollout_policy(auto_reset=True)",
                    "rollout_population", "ik(stage)+step"):   # (an env ik held is handed its own pose: it stays where it is)
            for a in committed(op):
                self.step(a, auto_reset="True" in op)
        elif op == "set(F_GOALS)":
            o.goals = d.poses[s].astype(np.float64)
            self._posed()
        elif op == "set(F_POINTS)":
            o.points = d.pts_set[s].astype(np.float64)
        elif op == "set(F_ALIVE)":
            o.alives = d.alive[s].astype(bool)
        elif op == "set_state":
            sv = self.saved
            o.goals, o.points, o.alives, o.total_reward = sv["goals"].copy(), sv["points"].copy(), sv["alives"].copy(), sv["total"].copy()
            self.episodes, self.done_state = sv["episodes"].copy(), sv["done_state"].copy()
            self.guarded = self.guarded | sv["guarded"]      # (the state is the saved one; the union is the cautious choice)
            self._posed()
        elif op == "observe":
            o.get_observations()                             # zeroes the targets that are dead (manytor.py:148)
        elif op == "check_done":
            pre_alive = o.alives.copy()
            o.is_done()
            pm = np.where(pre_alive, o.pickup_margin, np.inf).min(axis=1)
            self.guarded |= pm < self.GUARD
            self.done_state = (~o.alives.any(axis=1)).astype(np.uint8)
        elif op in NOTHING:
            pass
        else:
            raise KeyError(op)
