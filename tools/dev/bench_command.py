#!/usr/bin/env python3
"""What velocity commands cost beside a step and beside the same work in eager torch ops: solorl_commands with the observation copy
([N, 76] rows widened to [N, 79], the example ranges of configs/commands_walk12.yaml, the restart flags of a running rollout) and one
eagerly launched step, on the fp32 Solo12 walk workload at 4096 and 65 536 envs, all in one run.  Both read paths of the kernel are
timed (obs_in 16-byte aligned: 16-byte loads; offset by one float: word by word), and the no-observation form.  The torch formulation is
what a user would write today: a countdown tensor, `rand` for the draws, `where` for the envs that draw, the zero command and the
deadband, and `cat` for the wide rows -- fp32 draws from torch's generator, no per-env stream.  Device events around ONE call per timed
repeat; the figure is the median of `--repeats` repeats after `--warmup` untimed ones.

Then the PPO loop (`--train-updates` > 1): train_ppo.py's train() in this process, README recipe shape (4096 envs, T = 400, 5 epochs x 50
mini-batches of 32 768, HIP graphs), without and with --commands configs/commands_walk12.yaml, alternating, `--train-repeats` times each;
env-steps/s over the updates after the first one (which holds the captures).  With commands the policy runs as a launch of its own.  Once
at the recipe's one history level (79 words: no policy kernels, the PyTorch path) and once without history (41 words: on the kernels).

Nothing is gated; writes `--out` (default profiles/r21_command.json).

    python tools/dev/bench_command.py [--out profiles/r21_command.json] [--sizes 4096 65536] [--train-updates 6]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
COMMAND_FILE = os.path.join(ROOT, "configs", "commands_walk12.yaml")


def train_rate(flags, updates, history=1, N=4096, T=400):
    """env-steps/s of updates 2 .. `updates` of one train() run (log records: cumulative steps and their rate since the start)"""
    import train_ppo
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo.train import train
    argv = ["--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", str(N), "--num-steps", str(T),
            "--use-gae", "--use-linear-lr-decay", "--ppo-epoch", "5", "--mini-batch-size", "32768", "--num-env-steps", str(N * T * updates),
            "--log-interval", "1"]
    if flags:
        argv += ["--commands", COMMAND_FILE]
    args = train_ppo.get_ppo_args(argv)
    args.cuda = True
    config = load_yaml(args.config_file)
    config["task"] = args.task
    config["num_history_stack"] = history
    if args.commands is not None:
        args.commands = train_ppo.load_commands(args.commands)
    _, hist = train(args, config)
    t = [h["timesteps"] / h["fps"] for h in hist]                 # seconds since the loop's start at each record
    return (hist[-1]["timesteps"] - hist[0]["timesteps"]) / (t[-1] - t[0])


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join("profiles", "r21_command.json"))
    p.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--train-updates", type=int, default=6, help="updates per train() run of the PPO-loop comparison (0 = skip it)")
    p.add_argument("--train-repeats", type=int, default=2)
    p.add_argument("--train-history", type=int, nargs="+", default=[1, 0],
                   help="num_history_stack of the PPO-loop comparisons: 1 is the recipe (76 -> 79 words: the 79-wide policy has no kernels and runs "
                        "on the PyTorch path), 0 its zero-history form (38 -> 41 words: both policies on the kernels)")
    a = p.parse_args(argv)

    import torch
    import yaml
    from solorl_amd import command
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

    result = dict(workload="solo12 walk fp32, num_history_stack 1 (observation rows [N, 76] -> [N, 79])", repeats=a.repeats, warmup=a.warmup,
                  commands="configs/commands_walk12.yaml", device=torch.cuda.get_device_name(0), sizes={})
    ranges = command.ranges_from_dict(yaml.safe_load(open(COMMAND_FILE)))
    for N in a.sizes:
        cfg = default_config(ROBOT_SOLO12, TASK_WALK); cfg.num_history_stack = 1
        env = SoloVecEnv(cfg, N, device=dev, seed=1)
        env.reset()
        g = torch.Generator(device=dev); g.manual_seed(0)
        act = (torch.rand(N, env.act_dim, device=dev, generator=g) * 2 - 1) * 0.5
        for _ in range(20):                                     # contacts, history: a state as a rollout has it
            o, _, done, _ = env.step_inplace(act)
        obs, done = o.clone(), done.clone()
        D = obs.shape[1]
        r = {}
        r["step"] = timed(lambda: env.step_inplace(act))        # (nothing set: the step launch alone)
        params = command.make_params(1, 0, D, **ranges)
        mem = command.CommandMem(N, dev)
        wide = torch.empty((N, D + 3), dtype=torch.float32, device=dev)
        cmd_out = torch.empty((N, 3), dtype=torch.float64, device=dev)
        r["commands"] = timed(lambda: command.commands(params, mem, obs, out=wide, restart=done))
        r["commands_with_cmd_out"] = timed(lambda: command.commands(params, mem, obs, out=wide, cmd_out=cmd_out, restart=done))
        view = torch.zeros(N * D + 4, device=dev)[1:1 + N * D].view(N, D)
        view.copy_(obs)
        r["commands_unaligned_obs_in"] = timed(lambda: command.commands(params, mem, view, out=wide, restart=done))      # the word-by-word read path
        every = torch.ones_like(done)
        r["commands_every_env_draws"] = timed(lambda: command.commands(params, mem, obs, out=wide, restart=every))
        r["commands_no_observation"] = timed(lambda: command.commands(params, mem, restart=done))
        r["torch_cat_alone"] = timed(lambda: torch.cat([obs, wide[:, D:]], dim=1))                                        # the copy by itself
        lo = torch.tensor(list(params.lo), device=dev)
        width = torch.tensor(list(params.hi), device=dev) - lo
        scale = torch.tensor(list(params.obs_scale), device=dev)
        state = dict(cmd=torch.zeros(N, 3, device=dev), countdown=torch.ones(N, dtype=torch.int32, device=dev))
        span = params.interval_max - params.interval_min + 1

        def torch_commands():
            cd = state["countdown"] - 1
            now = (done != 0) | (cd == 0)
            c = lo + torch.rand(N, 3, device=dev) * width
            c = torch.where(torch.rand(N, 1, device=dev) < params.zero_prob, torch.zeros_like(c), c)
            short = (c[:, :2] * c[:, :2]).sum(1, keepdim=True) < params.min_lin_norm ** 2
            c = torch.cat([torch.where(short, torch.zeros_like(c[:, :2]), c[:, :2]), c[:, 2:]], dim=1)
            state["cmd"] = torch.where(now.unsqueeze(-1), c, state["cmd"])
            state["countdown"] = torch.where(now, params.interval_min + torch.randint(0, span, (N,), device=dev, dtype=torch.int32), cd)
            return torch.cat([obs, state["cmd"] * scale], dim=1)
        r["torch_commands"] = timed(torch_commands)
        for k in ("commands", "commands_with_cmd_out", "commands_unaligned_obs_in", "commands_every_env_draws", "commands_no_observation", "torch_commands",
                  "torch_cat_alone"):
            r[k + "_over_step"] = r[k]["median_ms"] / r["step"]["median_ms"]
        r["torch_commands_over_kernel"] = r["torch_commands"]["median_ms"] / r["commands"]["median_ms"]
        r["torch_cat_alone_over_kernel"] = r["torch_cat_alone"]["median_ms"] / r["commands"]["median_ms"]
        r["moved_bytes"] = N * (D + D + 3) * 4 + N * 64
        r["commands_GB_per_s"] = r["moved_bytes"] / (r["commands"]["median_ms"] * 1e-3) / 1e9
        result["sizes"][str(N)] = r
        print(N, json.dumps(r), flush=True)
        env.close()
    for history in (a.train_history if a.train_updates > 1 else ()):
        runs = {"plain": [], "commands": []}
        for rep in range(a.train_repeats):                      # alternating: the same build, the same session
            for name in ("plain", "commands"):
                runs[name].append(train_rate(name != "plain", a.train_updates, history))
                print("train history", history, name, runs[name][-1], flush=True)
        med = {k: statistics.median(v) for k, v in runs.items()}
        width = 38 * (1 + history)
        result["ppo_loop" if history == 1 else "ppo_loop_history%d" % history] = dict(
            shape="4096 envs, T = 400, 5 epochs x 50 mini-batches of 32768, HIP graphs, num_history_stack %d; env-steps/s over updates 2..%d" % (history, a.train_updates),
            flags="--commands configs/commands_walk12.yaml: the policy reads %d words instead of %d and runs as a launch of its own (the policy "
                  "tail of the step kernel is given up), plus the command launch per step; %s" % (
                      width + 3, width, "no policy kernels at 79 words: act and the mini-batch step run on the PyTorch path" if history == 1 else
                      "both widths have policy kernels"),
            env_steps_per_s=runs, median=med, commands_over_plain=med["commands"] / med["plain"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
