#!/usr/bin/env python3
"""What early termination costs beside a step: solorl_terminate alone, the chain a step gains while a termination is set (get_states +
solorl_terminate + solorl_reset_masked), one eagerly launched step of the same run, and the same rules as eager torch ops on get_states
rows followed by reset_masked() -- on the fp32 Solo12 walk workload at 4096 and 65 536 envs, all in one run.  Device events around ONE
call per timed repeat; the figure is the median of `--repeats` repeats after `--warmup` untimed ones.  Rules as
configs/termination_walk12.yaml sets them (base and shoulder contact, 60 degrees of tilt, min_steps 2); the state is the one 20 random
steps leave, restored in front of every group of calls, so some envs are on the ground and the reset has work to do.

Then the PPO loop (`--train-updates` > 0): train_ppo.py's train() in this process, README recipe shape (4096 envs, T = 400, 5 epochs x
50 mini-batches of 32 768, HIP graphs), without a termination, with --termination configs/termination_walk12.yaml, and without one
under SOLORL_STEP_ACT=0 (the policy tail given up, which a termination forces: that share of the loss is not the chain's), alternating,
`--train-repeats` times each; env-steps/s over the updates after the first one (which holds the captures), from the loop's own log
records.

Nothing is gated; writes `--out` (default profiles/r22_terminate.json).

    python tools/dev/bench_terminate.py [--out profiles/r22_terminate.json] [--sizes 4096 65536] [--train-updates 6]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
RULES_FILE = os.path.join(ROOT, "configs", "termination_walk12.yaml")


def train_rate(variant, updates, N=4096, T=400):
    """env-steps/s of updates 2 .. `updates` of one train() run (log records: cumulative steps and their rate since the start), and the
    share of the finished episodes a rule ended"""
    import train_ppo
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo.train import train
    argv = ["--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", str(N), "--num-steps", str(T),
            "--use-gae", "--use-linear-lr-decay", "--ppo-epoch", "5", "--mini-batch-size", "32768", "--num-env-steps", str(N * T * updates),
            "--log-interval", "1"]
    if variant == "termination":
        argv += ["--termination", RULES_FILE]
    args = train_ppo.get_ppo_args(argv)
    args.cuda = True
    config = load_yaml(args.config_file)
    config["task"] = args.task
    if args.termination is not None:
        args.termination = train_ppo.load_termination(args.termination, config)
    old = os.environ.get("SOLORL_STEP_ACT")
    if variant == "plain_no_policy_tail":
        os.environ["SOLORL_STEP_ACT"] = "0"
    try:
        _, hist = train(args, config)
    finally:
        if variant == "plain_no_policy_tail":
            if old is None:
                del os.environ["SOLORL_STEP_ACT"]
            else:
                os.environ["SOLORL_STEP_ACT"] = old
    t = [h["timesteps"] / h["fps"] for h in hist]                 # seconds since the loop's start at each record
    eps = sum(h.get("term/episodes", 0) for h in hist)
    early = sum(h["term/early"] * h["term/episodes"] for h in hist if h.get("term/episodes", 0)) / eps if eps else None
    return (hist[-1]["timesteps"] - hist[0]["timesteps"]) / (t[-1] - t[0]), early, sum(h["episodes"] for h in hist)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join("profiles", "r22_terminate.json"))
    p.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--train-updates", type=int, default=6, help="updates per train() run of the PPO-loop comparison (0 = skip it)")
    p.add_argument("--train-repeats", type=int, default=2)
    a = p.parse_args(argv)

    import torch
    from solorl_amd.config import default_config, load_yaml, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.termination import make_termination, terminate
    from solorl_amd.vec_env import SoloVecEnv
    dev = torch.device("cuda:0")
    rules = load_yaml(RULES_FILE)

    def timed(fn, before=None):
        ms = []
        for r in range(a.warmup + a.repeats):
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))

    result = dict(workload="solo12 walk fp32, num_history_stack 1", repeats=a.repeats, warmup=a.warmup, rules=rules,
                  device=torch.cuda.get_device_name(0), sizes={})
    for N in a.sizes:
        cfg = default_config(ROBOT_SOLO12, TASK_WALK); cfg.num_history_stack = 1
        env = SoloVecEnv(cfg, N, device=dev, seed=1)
        env.reset()
        g = torch.Generator(device=dev); g.manual_seed(0)
        act = torch.rand(N, env.act_dim, device=dev, generator=g) * 2 - 1
        for _ in range(20):                                     # contacts, history, robots on the ground: a state as a rollout has it
            env.step_inplace(act)
        rows = env.get_states()
        saved = rows.clone()
        P = make_termination(cfg, **rules)
        done, rew, fired = (torch.zeros(N, dtype=torch.uint8, device=dev), torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev))
        stats = torch.zeros(5, N, device=dev)
        restore = lambda: (env.set_states(saved), done.zero_())  # every timed call sees the same state and no env already ended
        r = {}
        r["get_states"] = timed(lambda: env.get_states(out=rows), restore)
        r["terminate"] = timed(lambda: terminate(cfg, P, rows, done, rew, fired, info=env._info_c, term_stats=stats), restore)
        r["fired_share"] = float((fired != 0).double().mean())
        env.set_termination(**rules)
        r["added_chain"] = timed(lambda: env._terminate(env._obs_engine, rew, done), restore)
        env.set_termination(None)
        env.set_states(saved)
        r["step"] = timed(lambda: env.step_inplace(act))        # (no termination set: the step launch alone)

        # the same rules as eager torch ops on the rows, then reset_masked()
        prims = torch.tensor([q for q in range(24) if (P.contact_prims >> q) & 1], device=dev, dtype=torch.int32)

        def torch_rules():
            s = env.get_states(out=rows)
            up_z = 1.0 - 2.0 * (s.quat[:, 0] * s.quat[:, 0] + s.quat[:, 1] * s.quat[:, 1])
            touch = ((s.contact_mask.unsqueeze(1) >> prims) & 1).bool() & (s.lambda_prev[:, prims.long()] / cfg.sim_dt >= P.contact_force_min)
            end = ((up_z < P.min_up_z) | touch.any(dim=1)) & (s.timestep >= P.min_steps) & (done == 0)
            rew.masked_fill_(end, P.terminal_reward)
            done.masked_fill_(end, 1)
            env.reset_masked(end)
        r["torch_rules_and_reset_masked"] = timed(torch_rules, restore)
        r["added_chain_over_step"] = r["added_chain"]["median_ms"] / r["step"]["median_ms"]
        r["terminate_over_step"] = r["terminate"]["median_ms"] / r["step"]["median_ms"]
        r["torch_over_added_chain"] = r["torch_rules_and_reset_masked"]["median_ms"] / r["added_chain"]["median_ms"]
        result["sizes"][str(N)] = r
        print(N, json.dumps(r), flush=True)
        env.close()
    if a.train_updates > 1:
        names = ("plain", "termination", "plain_no_policy_tail")
        runs, early = {k: [] for k in names}, []
        for rep in range(a.train_repeats):                      # alternating: the same build, the same session
            for name in names:
                rate, share, episodes = train_rate(name, a.train_updates)
                runs[name].append(rate)
                if share is not None:
                    early.append(dict(share_of_episodes_ended_by_a_rule=share, episodes=episodes))
                print("train", name, rate, share, episodes, flush=True)
        med = {k: statistics.median(v) for k, v in runs.items()}
        result["ppo_loop"] = dict(shape="4096 envs, T = 400, 5 epochs x 50 mini-batches of 32768, HIP graphs; env-steps/s over updates 2..%d" % a.train_updates,
                                  env_steps_per_s=runs, median=med, termination_over_plain=med["termination"] / med["plain"],
                                  no_policy_tail_over_plain=med["plain_no_policy_tail"] / med["plain"],
                                  termination_over_no_policy_tail=med["termination"] / med["plain_no_policy_tail"], termination_runs=early)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
