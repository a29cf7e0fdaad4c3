"""eval_ppo.py --push-interval / --push-max-vel: the trained Solo12 walk fixture policy evaluated under base-velocity kicks
(SoloVecEnv.push).  No success-rate threshold: what a 0.5 m/s kick does to that gait is recorded, not required."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checkpoint_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("walk12_ckpt")
    sd = torch.load(os.path.join(ROOT, "tests", "golden", "policies", "walk12.pt"), map_location="cpu", weights_only=False)
    torch.save({"update": 0, "state_dict": sd, "ob_rms": None}, os.path.join(str(d), "solo.pt"))
    return str(d)


def _run(checkpoint_dir, *extra):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import eval_ppo
    return eval_ppo.main(["--checkpoint-dir", checkpoint_dir, "--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk",
                          "--num-agents", "16", "--num-runs", "4", "--deterministic"] + list(extra))


def test_push_interval_zero_is_the_plain_evaluation(gpu_device, checkpoint_dir):
    plain = _run(checkpoint_dir)
    off = _run(checkpoint_dir, "--push-interval", "0")
    assert plain == off and plain["episodes"] >= 4
    assert _run(checkpoint_dir, "--push-interval", "0", "--push-max-vel", "0.5") == plain


def test_evaluation_under_pushes_finishes_with_finite_statistics(gpu_device, checkpoint_dir):
    r = _run(checkpoint_dir, "--push-interval", "10", "--push-max-vel", "0.5")
    print("eval under 0.5 m/s pushes every 10 steps:", r)
    assert r["episodes"] >= 4
    assert all(math.isfinite(float(r[k])) for k in ("mean_length", "mean_reward", "mean_success"))
    assert 1 <= r["mean_length"] <= 400 and 0.0 <= r["mean_success"] <= 1.0
