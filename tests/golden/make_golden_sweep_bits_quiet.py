"""Second set of bit pins of the team-mode step (tests/test_sweep_bits_quiet_gpu.py): cases in which teams become quiet EARLY and often,
i.e. in which the sweep's exit bookkeeping -- the cold block that decides which team leaves, and publishes its result -- runs in a
large share of the sweeps.  tests/golden/sweep_bits.json pins the thrashing robots of the bench; here:

  solo12_stand_pd_n9      Solo12 stand under PD control with the gains of configs/basic_pd.yaml ([5, 0.2]): 9 envs (three wavefronts,
                          the last with one team), 60 control steps, references = the crouch + a seeded +-0.02 rad per env and joint.
                          A standing robot's solves mostly end early (fixture: "mean_sweeps_oracle" = 17.6, the fp64 CPU oracle's sweeps
                          per solve over every sub-step with rows on the same inputs -- a stand-in: the plain library does not count
                          its sweeps) with 6.4 contacts on average, so its wavefronts run the heavy gated variants.  The kernel's
                          fp32 row loop on the CPU (tools/dev/k7_gate_share.py --case solo12_stand_pd_n9: the team sweep's rows,
                          order and K7 rule) gives the same 17.6 sweeps per solve, and 22 % of a wavefront's sweeps enter the cold block.
  solo12_pointgoal_n13    Solo12 pointgoal with seeded U(-1,1) torques: 13 envs (four wavefronts, the last with one team), 60 steps;
                          the robots fall, so resets happen inside the window ("resets": 28, and 28 on the CPU oracle); 14 % of an
                          unfinished env's sweeps are candidates for the cold block (same tool, --case solo12_pointgoal_n13).

    python tests/golden/make_golden_sweep_bits_quiet.py            # writes tests/golden/sweep_bits_quiet.json (needs the GPU)
    python tests/golden/make_golden_sweep_bits_quiet.py --check    # runs every case twice and compares, writes nothing

The hashes of the committed fixture were generated with the library built from commit d6e7947 ("Team PGS sweep: 35 fewer issue slots per sweep"),
BEFORE the K7 test of the cone sweeps' friction pairs moved into the cold block: that change, and any later one that is meant to leave
the arithmetic and the exit rule alone, has to reproduce these hashes.  Regenerate only for a change that is MEANT to alter either."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "sweep_bits_quiet.json")
SEED, STEPS = 5, 60
CASES = {"solo12_stand_pd_n9": ("stand_pd", 9), "solo12_pointgoal_n13": ("pointgoal", 13)}
CROUCH = np.array([0.0, 0.8, -1.6] * 4) / 10.0        # (PD references are action * 10 rad)


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def case_inputs(name):
    """(config, float32 actions [STEPS, N, 12])"""
    from solorl_amd.config import default_config, load_yaml, ROBOT_SOLO12, TASK_STAND, TASK_POINTGOAL, CONTROL_PD
    kind, N = CASES[name]
    rng = np.random.default_rng(SEED)
    if kind == "stand_pd":
        cfg = default_config(ROBOT_SOLO12, TASK_STAND)
        gains = load_yaml(os.path.join(ROOT, "configs", "basic_pd.yaml"))["gains"]
        cfg.control, cfg.kp, cfg.kd = CONTROL_PD, float(gains[0]), float(gains[1])
        acts = CROUCH[None, None, :] + 0.002 * rng.uniform(-1.0, 1.0, size=(STEPS, N, 12))
    else:
        cfg = default_config(ROBOT_SOLO12, TASK_POINTGOAL)
        acts = rng.uniform(-1.0, 1.0, size=(STEPS, N, 12))
    cfg.num_history_stack = 1
    return cfg, acts.astype(np.float32)


def run_case(name):
    """{array name: sha256} after STEPS control steps, plus the number of episode ends seen on the way"""
    import torch
    from solorl_amd.vec_env import SoloVecEnv
    cfg, acts = case_inputs(name)
    N = acts.shape[1]
    env = SoloVecEnv(cfg, N, device="cuda:0", seed=SEED)
    env.reset()
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


def oracle_sweeps(name):
    """mean sweep count of the fp64 CPU oracle's solves -- every sub-step with constraint rows of every control step and env -- on the same
    config, seed and actions (no GPU)"""
    from oracle.oracle_py import Oracle
    cfg, acts = case_inputs(name)
    N = acts.shape[1]
    o = Oracle(cfg, N, seed=SEED)
    o.reset()
    o.iteration_histogram(clear=True)           # (without the reset's settle steps)
    for k in range(STEPS):
        o.step(acts[k].astype(np.float64))
    h = o.iteration_histogram()
    return float((h * np.arange(len(h))).sum() / max(1, h.sum()))


def main():
    sys.path.insert(0, ROOT)
    a = {name: run_case(name) for name in CASES}
    if "--check" in sys.argv:
        b = {name: run_case(name) for name in CASES}
        print(json.dumps(a, indent=1))
        print("two runs agree" if a == b else "TWO RUNS DIFFER")
        return 0 if a == b else 1
    for name in CASES:
        a[name]["mean_sweeps_oracle"] = oracle_sweeps(name)
    with open(FIXTURE, "w") as f:
        json.dump(a, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(a, indent=1))
    print("wrote", FIXTURE)
    return 0


if __name__ == "__main__":
    sys.exit(main())
