"""Kernel setup happens at solorl_create (the SOLO_LDS_BASE checks, lane mode's dynamic-LDS limit), once per handle: what a handle
computes must not depend on which handles the process created before it.  Two handles made one after the other here are compared,
bitwise, with fresh processes that make only one of them (run as a script, this file is that process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (5, 67)
SEED = 6


def _make(N):
    import torch
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.vec_env import SoloVecEnv
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    cfg.num_history_stack = 1
    return SoloVecEnv(cfg, N, device=torch.device("cuda", 0), seed=SEED)


def _run(env):
    """reset, 3 steps, one step_n of K = 2 -> every output and the final state, as numpy arrays"""
    import torch
    N, A = env.nenvs, env.act_dim
    g = torch.Generator(); g.manual_seed(100 + N)
    acts = (torch.rand(5, N, A, generator=g) * 2 - 1).to(env.device)
    out = {"reset": env.reset()}
    for k in range(3):
        o, r, d, _ = env.step_inplace(acts[k].contiguous())
        out.update({"obs%d" % k: o.clone(), "rew%d" % k: r.clone(), "done%d" % k: d.clone()})
    o, r, d, _ = env.step_n_inplace(acts[3:].contiguous())
    out.update(obs_n=o.clone(), rew_n=r.clone(), done_n=d.clone(), state=env.get_states().bytes())
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.gpu
def test_outputs_do_not_depend_on_creation_order(gpu_device, tmp_path, monkeypatch):
    import torch
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    children = [subprocess.Popen([sys.executable, os.path.abspath(__file__), str(N), str(tmp_path / ("%d.npz" % N))], env=env,
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for N in SIZES]
    handles = [_make(N) for N in SIZES]                 # one after the other, both alive
    here = [_run(h) for h in handles]
    # lane mode: its create raises the step kernel's dynamic-LDS limit (a small batch asks for a whole CU's LDS per workgroup)
    monkeypatch.setenv("SOLORL_TEAM", "0")
    lane = _make(5)
    monkeypatch.delenv("SOLORL_TEAM")
    assert lane.get_property("lanes_per_env") == 1 and handles[0].get_property("lanes_per_env") == 16
    lane.reset()
    o, r, d, _ = lane.step_inplace(torch.zeros(5, 12, device=gpu_device))
    assert torch.isfinite(o).all() and torch.isfinite(r).all()
    for N, child, got in zip(SIZES, children, here):
        log, _ = child.communicate(timeout=300)
        assert child.returncode == 0, log[-4000:]
        want = np.load(tmp_path / ("%d.npz" % N))
        assert sorted(want.files) == sorted(got)
        for k in want.files:
            assert want[k].shape == got[k].shape and want[k].dtype == got[k].dtype, (N, k)
            assert np.array_equal(want[k].view(np.uint8), got[k].view(np.uint8)), (N, k)      # bitwise
        assert np.isfinite(got["obs_n"]).all() and got["obs_n"].shape == (2, N, 76)
    for h in handles + [lane]:
        h.close()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    np.savez(sys.argv[2], **_run(_make(int(sys.argv[1]))))
