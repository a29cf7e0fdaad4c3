"""eval_ppo.py --gait-metrics on the trained walk12 fixture policy (tests/golden/policies/walk12.pt), 64 envs, 50 control steps: every
metric is finite, duty factors lie in [0, 1], and the --dump file holds env 0's foot positions and forces from the batched call."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gait_metrics_and_dump(tmp_path):
    sd = torch.load(os.path.join(ROOT, "tests", "golden", "policies", "walk12.pt"), map_location="cpu", weights_only=True)
    torch.save({"state_dict": sd}, str(tmp_path / "solo.pt"))
    sys.path.insert(0, ROOT)
    import eval_ppo
    T, dump = 50, str(tmp_path / "traj.npz")
    r = eval_ppo.main(["--checkpoint-dir", str(tmp_path), "--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk",
                       "--num-agents", "64", "--num-runs", "100000", "--max-steps", str(T), "--deterministic", "--gait-metrics", "--dump", dump])
    g = r["gait"]
    assert g["steps"] == T
    per_foot = ("duty_factor", "mean_force", "peak_force", "slip_distance", "peak_clearance")
    for k in per_foot:
        assert len(g[k]) == 4 and np.isfinite(g[k]).all(), (k, g[k])
        assert (np.asarray(g[k]) >= 0).all(), (k, g[k])
    assert np.isfinite(g["support_ratio"]) and g["support_ratio"] > 0
    assert all(0.0 <= d <= 1.0 for d in g["duty_factor"])
    assert all(p >= m for p, m in zip(g["peak_force"], g["mean_force"]))
    assert max(g["duty_factor"]) > 0 and max(g["peak_force"]) > 0          # a walking robot touches the ground
    z = np.load(dump)
    assert z["foot_pos"].shape == (T, 4, 3) and z["foot_force"].shape == (T, 4) and z["q"].shape[0] == T
    assert np.isfinite(z["foot_pos"]).all() and np.isfinite(z["foot_force"]).all() and (z["foot_force"] >= 0).all()
    # the feet of env 0 hang below its base when it starts
    assert (z["foot_pos"][0, :, 2] < z["pos"][0, 2]).all()
