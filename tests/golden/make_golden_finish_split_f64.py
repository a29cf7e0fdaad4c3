"""Bit pin of the fp64 team-mode step with heavy and empty teams (tests/test_finish_split_gpu.py::test_fp64_kernels_are_the_parents):
sha256 of what 20 control steps of seeded U(-1,1) actions leave behind on 5 Solo12 envs, three of them lying on folded legs (8
contacts and limit rows: 17 rows or more) and two falling freely (no rows).

    python tests/golden/make_golden_finish_split_f64.py            # writes tests/golden/finish_split_f64.json (needs the GPU)
    python tests/golden/make_golden_finish_split_f64.py --check    # runs the case twice and compares, writes nothing

The committed fixture was generated with the library built from commit cafd9b5 ("Random base kicks on the device"), the parent of the
commit that split the duo kernel's row finish between its two wavefronts: the fp64 kernels are classic kernels, share the row finish's
and the sweeps' source with the duo kernel, and must come out of such a change as they went in.  A change that is MEANT to alter the
fp64 step's rounding regenerates the fixture deliberately and says so."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "finish_split_f64.json")
SEED, STEPS, N = 3, 20, 5
AIR, LYING = (0, 3), (1, 2, 4)
LYING_Z = (0.020, 0.025)


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def run_case():
    """{array name: sha256} after STEPS control steps, the contacts per env after the first one"""
    import torch
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK, PRECISION_F64
    from solorl_amd.vec_env import SoloVecEnv
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    cfg.num_history_stack = 1; cfg.precision = PRECISION_F64; cfg.disable_termination = 1
    env = SoloVecEnv(cfg, N, device="cuda:0", seed=SEED)
    assert env.get_property("f64") == 1
    env.reset()
    s = env.get_states()
    ql = float(env.cfg.joint_limit)
    for i in AIR + LYING:
        s.lin_vel[i] = 0; s.ang_vel[i] = 0; s.qd[i] = 0
    for i in AIR:
        s.pos[i, 2] = 1.0
    for k, i in enumerate(LYING):
        s.pos[i, 2] = LYING_Z[k % len(LYING_Z)]
        s.quat[i] = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)
        s.q[i, :12] = torch.tensor([0.0, ql, -ql] * 4, dtype=torch.float64)
        s.lambda_prev[i] = 0
    env.set_states(s)
    acts = np.random.default_rng(SEED).uniform(-1.0, 1.0, size=(STEPS, N, env.act_dim)).astype(np.float32)
    acts = torch.from_numpy(acts).to("cuda:0")
    first = None
    for k in range(STEPS):
        obs, rew, done, _ = env.step(acts[k])
        if k == 0:
            first = [bin(int(v) & 0xFFFFFF).count("1") for v in env.get_states().contact_mask.cpu()]
    torch.cuda.synchronize()
    out = {"obs": _sha(obs.cpu().numpy().tobytes()), "reward": _sha(rew.cpu().numpy().tobytes()),
           "done": _sha(done.cpu().numpy().tobytes()), "states": _sha(env.get_states().bytes().cpu().numpy().tobytes()),
           "contacts_first_step": first}
    env.close()
    return out


def main():
    sys.path.insert(0, ROOT)
    a = run_case()
    if "--check" in sys.argv:
        b = run_case()
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
