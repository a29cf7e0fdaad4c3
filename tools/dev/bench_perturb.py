#!/usr/bin/env python3
"""What a device-side kick costs beside a step and beside push(): solorl_perturb with the interval (1, 1) -- every env kicked in every
call, the worst case -- and with (10, 20), SoloVecEnv.push with a ready-made kick tensor, get_states, and one eagerly launched step, on
the fp32 Solo12 walk workload at 4096 and 65 536 envs, all in one run.  Device events around ONE call per timed repeat; the figure is
the median of `--repeats` repeats after `--warmup` untimed ones.  Amplitudes as train_ppo.py --push-max-vel 0.5 --push-max-yaw-rate 0.5
sets them (x, y, yaw rate); kick_out is written as the vec-env has it written.

Then the PPO loop (`--train-updates` > 0): train_ppo.py's train() in this process, README recipe shape (4096 envs, T = 400, 5 epochs x
50 mini-batches of 32 768, HIP graphs), without and with --push-interval 10:20 --push-max-vel 0.5, alternating, `--train-repeats` times
each; env-steps/s over the updates after the first one (which holds the captures), from the loop's own log records.

Nothing is gated; writes `--out` (default profiles/r17_perturb.json).

    python tools/dev/bench_perturb.py [--out profiles/r17_perturb.json] [--sizes 4096 65536] [--train-updates 6]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def train_rate(push, updates, N=4096, T=400):
    """env-steps/s of updates 2 .. `updates` of one train() run (log records: cumulative steps and their rate since the start)"""
    import train_ppo
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo.train import train
    argv = ["--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", str(N), "--num-steps", str(T),
            "--use-gae", "--use-linear-lr-decay", "--ppo-epoch", "5", "--mini-batch-size", "32768", "--num-env-steps", str(N * T * updates),
            "--log-interval", "1"]
    if push:
        argv += ["--push-interval", "10:20", "--push-max-vel", "0.5"]
    args = train_ppo.get_ppo_args(argv)
    args.cuda = True
    config = load_yaml(args.config_file)
    config["task"] = args.task
    _, hist = train(args, config)
    t = [h["timesteps"] / h["fps"] for h in hist]                 # seconds since the loop's start at each record
    return (hist[-1]["timesteps"] - hist[0]["timesteps"]) / (t[-1] - t[0])


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join("profiles", "r17_perturb.json"))
    p.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--train-updates", type=int, default=6, help="updates per train() run of the PPO-loop comparison (0 = skip it)")
    p.add_argument("--train-repeats", type=int, default=2)
    a = p.parse_args(argv)

    import torch
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.vec_env import SoloVecEnv
    dev = torch.device("cuda:0")

    def timed(fn):
        ms = []
        for r in range(a.warmup + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))

    result = dict(workload="solo12 walk fp32, num_history_stack 1", repeats=a.repeats, warmup=a.warmup, amplitudes="lin (0.5, 0.5, 0), ang (0, 0, 0.5)",
                  device=torch.cuda.get_device_name(0), sizes={})
    for N in a.sizes:
        cfg = default_config(ROBOT_SOLO12, TASK_WALK); cfg.num_history_stack = 1
        env = SoloVecEnv(cfg, N, device=dev, seed=1)
        env.reset()
        g = torch.Generator(device=dev); g.manual_seed(0)
        act = (torch.rand(N, env.act_dim, device=dev, generator=g) * 2 - 1) * 0.5
        for _ in range(20):                                     # contacts, history: a state as a rollout has it
            env.step_inplace(act)
        rows = env.get_states()
        saved = rows.clone()
        dv = torch.zeros(N, 6, dtype=torch.float64, device=dev)
        dv[:, (0, 1, 5)] = (torch.rand(N, 3, dtype=torch.float64, device=dev, generator=g) * 2 - 1) * 0.5
        r = {}
        r["get_states"] = timed(lambda: env.get_states(out=rows))
        r["push"] = timed(lambda: env.push(dv))                 # get + two torch adds + set(vel), the kick ready-made
        env.set_states(saved)
        r["step"] = timed(lambda: env.step_inplace(act))        # (no perturbation set yet: the step launch alone)
        env.set_states(saved)
        env.set_perturbation(1, (0.5, 0.5, 0.0), (0.0, 0.0, 0.5))
        r["perturb_every_env"] = timed(env.perturb)
        env.set_states(saved)
        env.set_perturbation((10, 20), (0.5, 0.5, 0.0), (0.0, 0.0, 0.5))
        r["perturb_10_20"] = timed(env.perturb)
        r["kicks_per_env_in_the_10_20_window"] = float(env.perturbation_state()[1].double().mean()) / (a.warmup + a.repeats)
        for k in ("perturb_every_env", "perturb_10_20"):
            r[k + "_over_step"] = r[k]["median_ms"] / r["step"]["median_ms"]
            r[k + "_over_push"] = r[k]["median_ms"] / r["push"]["median_ms"]
        r["push_over_step"] = r["push"]["median_ms"] / r["step"]["median_ms"]
        result["sizes"][str(N)] = r
        print(N, json.dumps(r), flush=True)
        env.close()
    if a.train_updates > 1:
        runs = {"plain": [], "push_10_20": []}
        for rep in range(a.train_repeats):                      # alternating: the same build, the same session
            for name in ("plain", "push_10_20"):
                runs[name].append(train_rate(name != "plain", a.train_updates))
                print("train", name, runs[name][-1], flush=True)
        med = {k: statistics.median(v) for k, v in runs.items()}
        result["ppo_loop"] = dict(shape="4096 envs, T = 400, 5 epochs x 50 mini-batches of 32768, HIP graphs; env-steps/s over updates 2..%d" % a.train_updates,
                                  env_steps_per_s=runs, median=med, push_over_plain=med["push_10_20"] / med["plain"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
