#!/usr/bin/env python3
"""What observation noise and actuation cost beside a step, beside solorl_perturb and beside the same work in eager torch ops:
solorl_obs_noise on the [N, 76] observation rows (the example table of configs/noise_solo.yaml), solorl_actuate with delays 0..3 and a
20 % gain range, solorl_perturb with the interval (10, 20) and one eagerly launched step, on the fp32 Solo12 walk workload at 4096 and
65 536 envs, all in one run.  The torch formulations are what a user would write today: `obs + (rand_like(obs) * 2 - 1) * scale`, and a
four-level list of action tensors shifted per call with `where(done)` restarting the finished envs (fixed latency 2, one gain tensor
-- less than the kernel does: no per-env latency, no per-episode redraw).  Device events around ONE call per timed repeat; the figure is
the median of `--repeats` repeats after `--warmup` untimed ones.

Then the PPO loop (`--train-updates` > 0): train_ppo.py's train() in this process, README recipe shape (4096 envs, T = 400, 5 epochs x
50 mini-batches of 32 768, HIP graphs), without and with --obs-noise configs/noise_solo.yaml --action-delay 0:3 --motor-gain-range 0.2,
alternating, `--train-repeats` times each; env-steps/s over the updates after the first one (which holds the captures).

Then (`--eval`) the walk12 fixture policy under eval_ppo.py, 256 envs, deterministic: success and episode length at delays 0..3, and
under the example noise table at x1 and x2.  A measurement of that fixture's robustness, nothing more.

Nothing is gated; writes `--out` (default profiles/r20_channel.json).

    python tools/dev/bench_channel.py [--out profiles/r20_channel.json] [--sizes 4096 65536] [--train-updates 6] [--eval]"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
NOISE_FILE = os.path.join(ROOT, "configs", "noise_solo.yaml")


def train_rate(flags, updates, N=4096, T=400):
    """env-steps/s of updates 2 .. `updates` of one train() run (log records: cumulative steps and their rate since the start)"""
    import train_ppo
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo.train import train
    argv = ["--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", str(N), "--num-steps", str(T),
            "--use-gae", "--use-linear-lr-decay", "--ppo-epoch", "5", "--mini-batch-size", "32768", "--num-env-steps", str(N * T * updates),
            "--log-interval", "1"]
    if flags:
        argv += ["--obs-noise", NOISE_FILE, "--action-delay", "0:3", "--motor-gain-range", "0.2"]
    args = train_ppo.get_ppo_args(argv)
    args.cuda = True
    config = load_yaml(args.config_file)
    config["task"] = args.task
    if args.obs_noise is not None:
        args.obs_noise = train_ppo.load_obs_noise(args.obs_noise, config)
    _, hist = train(args, config)
    t = [h["timesteps"] / h["fps"] for h in hist]                 # seconds since the loop's start at each record
    return (hist[-1]["timesteps"] - hist[0]["timesteps"]) / (t[-1] - t[0])


def evaluate(extra, workdir):
    """eval_ppo.py on the walk12 fixture, 256 envs, deterministic, one episode per env"""
    import torch
    import eval_ppo
    sd = torch.load(os.path.join(ROOT, "tests", "golden", "policies", "walk12.pt"), map_location="cpu", weights_only=False)
    torch.save({"update": 0, "state_dict": sd, "ob_rms": None}, os.path.join(workdir, "solo.pt"))
    r = eval_ppo.main(["--checkpoint-dir", workdir, "--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk",
                       "--num-agents", "256", "--num-runs", "256", "--deterministic"] + extra)
    return {k: r[k] for k in ("episodes", "mean_length", "mean_success", "mean_reward")}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join("profiles", "r20_channel.json"))
    p.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--train-updates", type=int, default=6, help="updates per train() run of the PPO-loop comparison (0 = skip it)")
    p.add_argument("--train-repeats", type=int, default=2)
    p.add_argument("--eval", action="store_true", help="the walk12 fixture under delays 0..3 and under the example noise table x1, x2")
    a = p.parse_args(argv)

    import torch
    import yaml
    from solorl_amd import channel
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

    result = dict(workload="solo12 walk fp32, num_history_stack 1 (observation rows [N, 76], action rows [N, 12])", repeats=a.repeats, warmup=a.warmup,
                  noise="configs/noise_solo.yaml", actuation="delay 0..3, gain range 0.2", device=torch.cuda.get_device_name(0), sizes={})
    groups = yaml.safe_load(open(NOISE_FILE))
    for N in a.sizes:
        cfg = default_config(ROBOT_SOLO12, TASK_WALK); cfg.num_history_stack = 1
        env = SoloVecEnv(cfg, N, device=dev, seed=1)
        obs = env.reset()
        g = torch.Generator(device=dev); g.manual_seed(0)
        act = (torch.rand(N, env.act_dim, device=dev, generator=g) * 2 - 1) * 0.5
        for _ in range(20):                                     # contacts, history: a state as a rollout has it
            o, _, done, _ = env.step_inplace(act)
        obs, done = o.clone(), done.clone()
        r = {}
        r["step"] = timed(lambda: env.step_inplace(act))        # (nothing set yet: the step launch alone)
        env.set_perturbation((10, 20), (0.5, 0.5, 0.0), (0.0, 0.0, 0.5))
        r["perturb_10_20"] = timed(env.perturb)
        env.set_perturbation(None)
        scale = channel.scales_from_dict(cfg, groups).to(dev)
        count = torch.zeros(N, dtype=torch.int32, device=dev)
        r["obs_noise"] = timed(lambda: channel.obs_noise(1, 0, scale, count, obs))
        view = torch.zeros(N * 76 + 4, device=dev)[1:1 + N * 76].view(N, 76)
        r["obs_noise_unaligned_rows"] = timed(lambda: channel.obs_noise(1, 0, scale, count, view))      # the word-by-word path
        r["torch_obs_noise"] = timed(lambda: obs.add_((torch.rand_like(obs) * 2 - 1) * scale))
        params = channel.make_actuation(1, 0, 12, (0, 3), 0.2)
        mem = channel.ActuatorMem(N, dev)
        applied = torch.empty_like(act)
        r["actuate"] = timed(lambda: channel.actuate(params, mem, act, out=applied, restart=done))
        every = torch.ones_like(done)
        r["actuate_every_env_restarts"] = timed(lambda: channel.actuate(params, mem, act, out=applied, restart=every))
        levels = [torch.zeros_like(act) for _ in range(4)]
        gain = 1 + (torch.rand_like(act) * 2 - 1) * 0.2

        def torch_actuate():
            restart = done.bool().unsqueeze(-1)
            delayed = torch.where(restart, act, levels[1])      # latency 2 for every env; a finished env holds its first action
            out = gain * delayed
            for k in range(3, 0, -1):
                levels[k] = torch.where(restart, act, levels[k - 1])
            levels[0] = act.clone()
            return out
        r["torch_actuate"] = timed(torch_actuate)
        for k in ("perturb_10_20", "obs_noise", "obs_noise_unaligned_rows", "torch_obs_noise", "actuate", "actuate_every_env_restarts", "torch_actuate"):
            r[k + "_over_step"] = r[k]["median_ms"] / r["step"]["median_ms"]
        r["torch_obs_noise_over_kernel"] = r["torch_obs_noise"]["median_ms"] / r["obs_noise"]["median_ms"]
        r["torch_actuate_over_kernel"] = r["torch_actuate"]["median_ms"] / r["actuate"]["median_ms"]
        result["sizes"][str(N)] = r
        print(N, json.dumps(r), flush=True)
        env.close()
    if a.train_updates > 1:
        runs = {"plain": [], "noise_delay_gain": []}
        for rep in range(a.train_repeats):                      # alternating: the same build, the same session
            for name in ("plain", "noise_delay_gain"):
                runs[name].append(train_rate(name != "plain", a.train_updates))
                print("train", name, runs[name][-1], flush=True)
        med = {k: statistics.median(v) for k, v in runs.items()}
        result["ppo_loop"] = dict(shape="4096 envs, T = 400, 5 epochs x 50 mini-batches of 32768, HIP graphs; env-steps/s over updates 2..%d" % a.train_updates,
                                  flags="--obs-noise configs/noise_solo.yaml --action-delay 0:3 --motor-gain-range 0.2 (with noise the policy "
                                        "runs as a launch of its own: two launches per step instead of one)",
                                  env_steps_per_s=runs, median=med, flags_over_plain=med["noise_delay_gain"] / med["plain"])
    if a.eval:
        ev = {}
        with tempfile.TemporaryDirectory() as d:
            for k in range(4):
                ev["delay_%d" % k] = evaluate(["--action-delay", str(k)], d)
                print("eval delay", k, ev["delay_%d" % k], flush=True)
            for factor in (1, 2):
                path = os.path.join(d, "noise_x%d.yaml" % factor)
                with open(path, "w") as f:
                    yaml.safe_dump(dict(groups={k: v * factor for k, v in groups["groups"].items()}, history=groups.get("history", 1.0)), f)
                ev["noise_x%d" % factor] = evaluate(["--obs-noise", path], d)
                print("eval noise x", factor, ev["noise_x%d" % factor], flush=True)
        result["walk12_fixture_eval"] = dict(shape="eval_ppo.py, 256 envs, one episode each, deterministic, seed 7", runs=ev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
