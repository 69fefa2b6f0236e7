"""bench.py without a GPU: a plain run's protocol (one region of exactly --steps steps, no laps, the same calls whatever the
pre-warm did) and --dump-outputs (float32 / float64 files, a fixed sample, bounded size), on a stand-in engine."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

torch = pytest.importorskip("torch")


class _Engine:
    """What bench.measure asks of an engine, recording every reset and rollout call; returns = steps since the last reset."""

    def __init__(self, n):
        self.n_envs, self.env_id_base = n, 0
        self.ret = torch.zeros(n)
        self.calls, self.laps = [], 0

    def reset_random(self, seed, episode):
        self.calls.append(("reset", seed, episode))
        self.ret.zero_()

    def rollout(self, steps, seed, step0):
        self.calls.append(("rollout", steps, seed, step0))
        self.ret += steps

    rollout_fused = rollout

    def gather_begin(self, out=None, field=None, snapshot=True):
        return self.ret.clone()

    gather_returns = gather_begin

    def gather_wait(self, host=False):
        return 0.0 if host else None

    def lap_begin(self):
        self.laps += 1

    def lap_end(self):
        pass

    def lap_times(self):
        return [0.01] * self.laps

    def timer_start(self):
        pass

    def timer_stop_async(self):
        pass

    def timer_read(self):
        return 0.5

    def sync(self):
        pass

    def total_reward(self):
        return self.ret.numpy()

    # per-env fields as the engine's getters return them (K = 7 targets, D = 4 joints)
    def obs(self):
        return np.arange(self.n_envs * 21, dtype=np.float32).reshape(self.n_envs, 21)

    def reward(self):
        return np.ones(self.n_envs, dtype=np.int32)

    def done(self):
        return np.zeros(self.n_envs, dtype=bool)

    def ee(self):
        return np.ones((self.n_envs, 3), dtype=np.float32)

    def goals(self):
        return np.ones((self.n_envs, 4), dtype=np.float32)

    def alives(self):
        return np.ones((self.n_envs, 7), dtype=bool)

    def points(self):
        return np.ones((self.n_envs, 7, 3), dtype=np.float32)


@pytest.mark.parametrize("steps,warmup,phase", [(20, 5, 0), (1000, 50, 0), (7, 0, 0), (20, 5, 10)])
def test_one_region_of_exactly_steps_without_laps_whatever_the_prewarm(steps, warmup, phase, monkeypatch):
    """repeats = 1, laps = False (a plain run): one region of exactly `steps` steps, no HIP-event laps; the calls from the
    restart on are the same for a short and a long pre-warm, so the outputs of the timed steps depend on the arguments only."""
    monkeypatch.setattr(bench.EpisodeLoop, "phase", phase)
    after = []
    for prewarm_s in (0.0, 0.05):
        eng = _Engine(64)
        res = bench.measure(bench.Fabric(), eng, 64, steps, warmup, 50, 0x5EED, repeats=1, prewarm_s=prewarm_s, laps=False)
        assert res["repeats"] == 1 and res["lapped_regions"] == 0 and eng.laps == 0
        assert res["step_us"] is None and res["ms_per_step_lapped_regions"] is None
        assert res["ms_per_step"] == pytest.approx(res["elapsed"] / steps * 1e3)
        assert res["value"] == pytest.approx(64 * steps / res["elapsed"])
        restart = max(i for i, c in enumerate(eng.calls) if c == ("reset", 0x5EED, 0))
        tail = eng.calls[restart:]
        # after the restart: the warm-up steps, the `phase` steps align() runs, then the timed steps -- and nothing else
        assert sum(c[1] for c in tail if c[0] == "rollout") == warmup + phase % res["episode_len"] + steps
        after.append((tail, res["returns"].tolist()))
    assert after[0] == after[1]


def test_dump_outputs_writes_float_arrays_of_a_fixed_sample(tmp_path):
    n = bench.DUMP_SAMPLE + 1000
    eng = _Engine(n)
    eng.ret += 3
    returns = np.arange(n, dtype=np.float32)
    shapes = bench.dump_outputs(str(tmp_path / "a"), eng, returns)
    bench.dump_outputs(str(tmp_path / "b"), eng, returns)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(name + ".npy" for name in shapes)
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(a, b)
        total += os.path.getsize(tmp_path / "a" / f)
    assert total <= 64 * 10 ** 6
    ids = np.load(tmp_path / "a" / "env_ids.npy")
    assert len(ids) == bench.DUMP_SAMPLE and np.all(np.diff(ids) > 0) and ids[-1] < n
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "obs.npy")[:, 0], ids * 21)     # the rows of the sampled envs
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "returns.npy"), returns)        # every env's return: small here
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "total_reward.npy"), 3)


def test_plain_and_full_options_are_there():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                         timeout=120, cwd=ROOT)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout
