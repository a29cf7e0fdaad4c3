"""Bit pins of the team-mode step (tests/test_sweep_bits_gpu.py): sha256 of what 80 control steps of seeded U(-1,1) actions leave behind.

    python tests/golden/make_golden_sweep_bits.py            # writes tests/golden/sweep_bits.json (needs the GPU)
    python tests/golden/make_golden_sweep_bits.py --check    # runs every case twice and compares, writes nothing

The committed fixture was generated with the library built from commit 17b5093 ("Add K-step launches: solorl_step_n and
solorl_rollout"), i.e. BEFORE the sweep loop of pgs_team_variant lost its non-arithmetic issue slots: that change, and any later one
that is meant to leave the arithmetic alone, has to reproduce these hashes.  The parity tests cannot stand in for this: a team that
leaves the sweep one iteration late moves a velocity by at most 3e-4 m/s.  A change that is MEANT to alter rounding (or the exit rule)
regenerates the fixture deliberately and says so.

Cases: Solo12 walk with 67 envs (17 wavefronts, the last with three teams and one idle) and Solo8 walk with 5 envs; random torques
make the robots fall, so resets happen inside the window ("resets" in the fixture counts them), and solves that never meet the K7
residual occur along the way."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "sweep_bits.json")
SEED, STEPS = 3, 80
CASES = {"solo12_walk_n67": ("solo12", 67), "solo8_walk_n5": ("solo8", 5)}


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def run_case(name):
    """{array name: sha256} after STEPS control steps, plus the number of episode ends seen on the way"""
    import torch
    from solorl_amd.config import default_config, ROBOT_SOLO8, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.vec_env import SoloVecEnv
    robot, N = CASES[name]
    cfg = default_config(ROBOT_SOLO12 if robot == "solo12" else ROBOT_SOLO8, TASK_WALK)
    cfg.num_history_stack = 1
    env = SoloVecEnv(cfg, N, device="cuda:0", seed=SEED)
    env.reset()
    acts = np.random.default_rng(SEED).uniform(-1.0, 1.0, size=(STEPS, N, env.act_dim)).astype(np.float32)
    acts = torch.from_numpy(acts).to("cuda:0")
    resets = 0
    for k in range(STEPS):
        obs, rew, done, _ = env.step(acts[k])
        resets += int(done.sum().item())
    torch.cuda.synchronize()
    out = {"obs": _sha(obs.cpu().numpy().tobytes()), "reward": _sha(rew.cpu().numpy().tobytes()),
           "done": _sha(done.cpu().numpy().tobytes()), "state_first": _sha(bytes(env.get_state(0))),
           "state_last": _sha(bytes(env.get_state(N - 1))), "resets": resets}
    env.close()
    return out


def main():
    sys.path.insert(0, ROOT)
    a = {name: run_case(name) for name in CASES}
    if "--check" in sys.argv:
        b = {name: run_case(name) for name in CASES}
        print(json.dumps(a, indent=1))
        print("two runs agree" if a == b else "TWO RUNS DIFFER")
        return 0 if a == b else 1
    with open(FIXTURE, "w") as f:
        json.dump(a, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE)
    return 0


if __name__ == "__main__":
    sys.exit(main())
