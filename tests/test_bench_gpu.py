"""bench.py end to end on the GPU: the plain run's line and --dump-outputs (the same arguments give the same outputs), and the
auxiliary legs behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args), env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_repeatable_dump(gpu_device, tmp_path):
    K = 20
    lines = [_bench("--steps", str(K), "--warmup", "5", "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for ln in lines:
        assert ln["steps"] == K and ln["warmup"] == 5 and ln["unit"] == "env-steps/s" and ln["dtype"] == "f32" and ln["higher_is_better"] is True
        assert ln["value"] == pytest.approx(4096 * 1e3 / ln["ms_per_step"], rel=1e-9)
        assert ln["roofline"]["kernel_ms_avg"] <= ln["ms_per_step"] * 1.001
        assert not {"f64", "ppo_loop", "cpu_baseline", "repeats_ms_per_step"} & set(ln), "auxiliary legs ran without --full"
    names = sorted(os.listdir(tmp_path / "a"))
    assert {"obs.npy", "reward.npy", "done.npy", "info_episode_length.npy"} <= set(names)
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32 and x.shape[0] == 4096 and np.all(np.isfinite(x))
        assert np.array_equal(x, y), "%s differs between two runs with the same arguments" % f
    assert np.load(tmp_path / "a" / "obs.npy").shape == (4096, 76)          # Solo12 walk, one history level


@pytest.mark.gpu
def test_full_bench_runs_the_auxiliary_legs(gpu_device):
    ln = _bench("--full", "--steps", "20", "--warmup", "5", "--ppo-steps", "8", "--ppo-epoch", "1", "--no-cpu-baseline")
    assert ln["aux_legs_complete"] is True and len(ln["repeats_ms_per_step"]) == 5
    assert "error" not in ln["f64"] and ln["f64"]["dtype"] == "f64" and ln["f64"]["value"] > 0
    assert "error" not in ln["ppo_loop"] and ln["ppo_loop"]["rollout_steps"] == 8 and ln["ppo_loop"]["env_steps_per_s"] > 0
