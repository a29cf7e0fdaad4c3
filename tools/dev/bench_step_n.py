"""K steps per launch (solorl_step_n / solorl_rollout) against one launch per step, on the bench workload: Solo12 walk, U(-1, 1)
actions, after the 450-step burn-in.

  open loop    per batch size and K: graph A = K x step_inplace into [K, N] rows, graph B = one step_n_inplace into the same rows;
               replays alternate A, B (median of --reps each) -> ms per step and M env-steps/s
  closed loop  the T = 400 rollout at the README recipe shape (configs/basic12.yaml as walk, 4096 envs): GraphedRollout(chunk = 400)
               against today's path (one solorl_step_act launch per step), alternating replays

  python tools/dev/bench_step_n.py [--sizes 1024,4096,8192,65536] [--ks 1,8,50,400] [--reps 5] [--out FILE.json]
One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    b.synchronize()
    return a.elapsed_time(b)


def open_loop(N, ks, reps):
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.vec_env import SoloVecEnv
    dev = torch.device("cuda:0")
    cfg = default_config(ROBOT_SOLO12, TASK_WALK); cfg.num_history_stack = 1
    env = SoloVecEnv(cfg, N, device=dev, seed=1)
    env.reset()
    g = torch.Generator(device=dev); g.manual_seed(0)
    for _ in range(450):
        env.step_inplace(torch.rand(N, 12, device=dev, generator=g) * 2 - 1)
    torch.cuda.synchronize()
    out = []
    for K in ks:
        acts = torch.rand(K, N, 12, device=dev, generator=g) * 2 - 1
        obs, rew, done = torch.empty(K, N, env.obs_dim, device=dev), torch.empty(K, N, device=dev), torch.empty(K, N, dtype=torch.uint8, device=dev)
        ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(ga):
            for k in range(K):
                env.step_inplace(acts[k], obs_out=obs[k], rew_out=rew[k], done_out=done[k])
        with torch.cuda.graph(gb):
            env.step_n_inplace(acts, obs_out=obs, rew_out=rew, done_out=done)
        ta, tb = [], []
        ga.replay(); gb.replay(); torch.cuda.synchronize()          # (warm)
        for _ in range(reps):
            ta.append(_timed(ga.replay)); tb.append(_timed(gb.replay))
        ma, mb = float(np.median(ta)), float(np.median(tb))
        row = dict(N=N, K=K, per_step_ms=ma / K, step_n_ms=mb / K, per_step_Msps=K * N / ma / 1e3, step_n_Msps=K * N / mb / 1e3,
                   speedup=ma / mb, replays_ms_per_step=[t / K for t in ta], replays_ms_step_n=[t / K for t in tb])
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.startswith("replays")}), file=sys.stderr, flush=True)
        out.append(row)
        del ga, gb
    env.close()
    return out


def closed_loop(N, T, reps):
    from solorl_amd.config import config_from_dict, load_yaml
    from solorl_amd.ppo import Policy, RolloutStorage
    from solorl_amd.ppo.graphs import GraphedRollout
    from solorl_amd.vec_env import Box, SoloVecEnv
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dev = torch.device("cuda:0")
    cfg = config_from_dict(load_yaml(os.path.join(root, "configs", "basic12.yaml")), task="walk")
    torch.manual_seed(0)
    pol = Policy((cfg.obs_dim,), Box(-np.ones(12), np.ones(12)), None, {"hidden_size": 64}).to(dev)
    runs = {}
    for name, chunk in (("step_act", 0), ("rollout", T)):
        env = SoloVecEnv(cfg, N, device=dev, seed=1)
        st = RolloutStorage(T, N, (cfg.obs_dim,), 12, dev)
        st.obs[0].copy_(env.reset())
        with torch.no_grad():
            pol.act(st.obs[0])
        roll = GraphedRollout(env, pol, st, T, chunk=chunk)
        roll()                                                     # capture + first replay (burn-in: T steps)
        st.reset(); roll()
        torch.cuda.synchronize()
        runs[name] = (env, st, roll)
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, (env, st, roll) in runs.items():
            st.reset()
            times[k].append(_timed(roll))
    a, b = float(np.median(times["step_act"])), float(np.median(times["rollout"]))
    assert runs["rollout"][2].windows == [T] and runs["step_act"][2].windows is None
    return dict(N=N, T=T, step_act_ms=a, rollout_ms=b, speedup=a / b, step_act_Msps=T * N / a / 1e3, rollout_Msps=T * N / b / 1e3,
                replays_step_act_ms=times["step_act"], replays_rollout_ms=times["rollout"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,8192,65536")
    ap.add_argument("--ks", default="1,8,50,400")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--closed-envs", type=int, default=4096)
    ap.add_argument("--no-closed", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = dict(open_loop=[], closed_loop=None, device=torch.cuda.get_device_name(0))
    for N in (int(x) for x in a.sizes.split(",") if x):
        res["open_loop"] += open_loop(N, [int(k) for k in a.ks.split(",") if k], a.reps)
    if not a.no_closed:
        res["closed_loop"] = closed_loop(a.closed_envs, 400, a.reps)
        print(json.dumps({k: v for k, v in res["closed_loop"].items() if not k.startswith("replays")}), file=sys.stderr, flush=True)
    txt = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt)
    print(txt)


if __name__ == "__main__":
    main()
