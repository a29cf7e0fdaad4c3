#!/usr/bin/env python3
"""What randomised initial states cost beside a step: solorl_randomize_reset alone, solorl_restart_history alone, the four-launch chain a
step gains while a reset randomization is set (get_states + solorl_randomize_reset + solorl_set_states + solorl_restart_history), one
eagerly launched step of the same run, and the same draws as eager torch ops on get_states + get_kinematics + set_states -- on the fp32
Solo12 walk workload at 4096 and 65 536 envs, all in one run.  Device events around ONE call per timed repeat; the figure is the median
of `--repeats` repeats after `--warmup` untimed ones.  Ranges as configs/reset_walk12.yaml sets them; the mask selects every fourth env
(the chain's cost in a step depends on how many envs finished: `--all` selects every env, as reset() does).

Then the PPO loop (`--train-updates` > 0): train_ppo.py's train() in this process, README recipe shape (4096 envs, T = 400, 5 epochs x
50 mini-batches of 32 768, HIP graphs), without the feature, with --reset-randomization configs/reset_walk12.yaml, and without it under
SOLORL_STEP_ACT=0 (the policy tail given up, which the feature forces: that share of the loss is not the chain's), alternating,
`--train-repeats` times each; env-steps/s over the updates after the first one (which holds the captures).

The kernel's registers, LDS and occupancy are read from the built code object.  Nothing is gated; writes `--out` (default
profiles/r23_reset_random.json).

    python tools/dev/bench_reset_random.py [--out profiles/r23_reset_random.json] [--sizes 4096 65536] [--train-updates 6]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
RANGES_FILE = os.path.join(ROOT, "configs", "reset_walk12.yaml")


def train_rate(variant, updates, N=4096, T=400):
    """env-steps/s of updates 2 .. `updates` of one train() run (log records: cumulative steps and their rate since the start)"""
    import train_ppo
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo.train import train
    argv = ["--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", str(N), "--num-steps", str(T),
            "--use-gae", "--use-linear-lr-decay", "--ppo-epoch", "5", "--mini-batch-size", "32768", "--num-env-steps", str(N * T * updates),
            "--log-interval", "1"]
    if variant == "reset_randomization":
        argv += ["--reset-randomization", RANGES_FILE]
    args = train_ppo.get_ppo_args(argv)
    args.cuda = True
    config = load_yaml(args.config_file)
    config["task"] = args.task
    if args.reset_randomization is not None:
        args.reset_randomization = train_ppo.load_reset_randomization(args.reset_randomization, config)
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
    return (hist[-1]["timesteps"] - hist[0]["timesteps"]) / (t[-1] - t[0]), sum(h["episodes"] for h in hist)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join("profiles", "r23_reset_random.json"))
    p.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--all", action="store_true", help="select every env instead of every fourth")
    p.add_argument("--train-updates", type=int, default=6, help="updates per train() run of the PPO-loop comparison (0 = skip it)")
    p.add_argument("--train-repeats", type=int, default=2)
    a = p.parse_args(argv)

    import torch
    from solorl_amd import _native, build, devcode
    from solorl_amd.config import default_config, load_yaml, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.reset_random import make_reset_randomization, randomize_reset
    from solorl_amd.state import SF_CONTACT, SF_JOINT_POS, SF_JOINT_VEL, SF_POSE, SF_VEL
    from solorl_amd.vec_env import SoloVecEnv
    dev = torch.device("cuda:0")
    ranges = load_yaml(RANGES_FILE)
    fields = SF_POSE | SF_VEL | SF_JOINT_POS | SF_JOINT_VEL | SF_CONTACT

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

    res = {k: v for k, v in devcode.kernel_resources(build.LIB).items() if "reset_rows_kernel" in k or "restart_history_kernel" in k}
    keep = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
    result = dict(workload="solo12 walk fp32, num_history_stack 1", repeats=a.repeats, warmup=a.warmup, ranges=ranges,
                  selected="every env" if a.all else "every fourth env", device=torch.cuda.get_device_name(0), sizes={},
                  kernels={k: {f: r[f] for f in keep if f in r} for k, r in res.items()})
    for N in a.sizes:
        cfg = default_config(ROBOT_SOLO12, TASK_WALK); cfg.num_history_stack = 1
        env = SoloVecEnv(cfg, N, device=dev, seed=1)
        env.reset()
        g = torch.Generator(device=dev); g.manual_seed(0)
        act = torch.rand(N, env.act_dim, device=dev, generator=g) * 2 - 1
        for _ in range(20):                                     # contacts, history: a state as a rollout has it
            env.step_inplace(act)
        rows = env.get_states()
        saved = rows.clone()
        mask = torch.ones(N, dtype=torch.uint8, device=dev) if a.all else (torch.arange(N, device=dev) % 4 == 0).to(torch.uint8)
        P = make_reset_randomization(cfg, 1, 0, **ranges)
        count = torch.zeros(N, dtype=torch.int32, device=dev)
        restore = lambda: (env.set_states(saved), rows.data.copy_(saved.data))     # every timed call sees the same state and rows
        L = _native.lib()
        r = {}
        r["get_states"] = timed(lambda: env.get_states(mask, out=rows), restore)
        r["randomize_reset"] = timed(lambda: randomize_reset(cfg, P, rows, count, mask=mask), restore)
        r["set_states"] = timed(lambda: env.set_states(rows, mask, fields), restore)
        r["restart_history"] = timed(lambda: _native.check(L.solorl_restart_history(env._h, C.c_void_p(mask.data_ptr()), C.c_void_p(env._obs_engine.data_ptr()),
                                                                                    env._stream())), restore)
        env.set_reset_randomization(**ranges)
        r["added_chain"] = timed(lambda: env._randomize(env._obs_engine, mask), restore)
        env.set_reset_randomization(None)
        env.set_states(saved)
        r["step"] = timed(lambda: env.step_inplace(act))        # (feature off: the step launch alone)

        # the same draws as eager torch ops on the rows: uniform offsets, the turn of the base, the height from get_kinematics
        sel = mask.bool()

        def quat_mul(p_, q_):
            px, py, pz, pw = p_.unbind(-1)
            qx, qy, qz, qw = q_.unbind(-1)
            return torch.stack([pw * qx + px * qw + py * qz - pz * qy, pw * qy - px * qz + py * qw + pz * qx, pw * qz + px * qy - py * qx + pz * qw,
                                pw * qw - px * qx - py * qy - pz * qz], dim=-1)

        def torch_draws():
            s = env.get_states(mask, out=rows)
            u = lambda *shape: torch.rand(*shape, device=dev, dtype=torch.float64, generator=g) * 2 - 1
            m = sel.unsqueeze(-1)
            s.q.add_(torch.where(m, u(N, 12) * ranges["joint_pos"], 0.0)).clamp_(-cfg.joint_limit, cfg.joint_limit)
            s.qd.add_(torch.where(m, u(N, 12) * ranges["joint_vel"], 0.0))
            s.lin_vel.add_(torch.where(m, u(N, 3) * ranges["lin_vel"], 0.0))
            s.ang_vel.add_(torch.where(m, u(N, 3) * ranges["ang_vel"], 0.0))
            ang = u(N, 3) * torch.tensor([ranges["yaw"], ranges["roll"], ranges["pitch"]], device=dev, dtype=torch.float64) * 0.5
            z = torch.zeros(N, device=dev, dtype=torch.float64)
            sn, cs = ang.sin(), ang.cos()
            q = quat_mul(torch.stack([z, z, sn[:, 0], cs[:, 0]], dim=-1), s.quat)
            q = quat_mul(quat_mul(q, torch.stack([sn[:, 1], z, z, cs[:, 1]], dim=-1)), torch.stack([z, sn[:, 2], z, cs[:, 2]], dim=-1))
            q = q / q.norm(dim=-1, keepdim=True)
            s.quat.copy_(torch.where(m, torch.where(q[:, 3:] < 0, -q, q), s.quat))
            zmin = env.get_kinematics(mask, states=s).prim_point[:, :, 2].min(dim=1).values
            s.pos[:, 2].add_(torch.where(sel, ranges["clearance"] - zmin, 0.0))
            s.lambda_prev.masked_fill_(m, 0.0)
            s.contact_mask.bitwise_and_(torch.where(sel, -16777216, -1).to(torch.int32))
            env.set_states(s, mask, fields)
            _native.check(L.solorl_restart_history(env._h, C.c_void_p(mask.data_ptr()), C.c_void_p(env._obs_engine.data_ptr()), env._stream()))
        r["torch_draws_and_kinematics"] = timed(torch_draws, restore)
        r["added_chain_over_step"] = r["added_chain"]["median_ms"] / r["step"]["median_ms"]
        r["randomize_reset_over_step"] = r["randomize_reset"]["median_ms"] / r["step"]["median_ms"]
        r["torch_over_added_chain"] = r["torch_draws_and_kinematics"]["median_ms"] / r["added_chain"]["median_ms"]
        result["sizes"][str(N)] = r
        print(N, json.dumps(r), flush=True)
        env.close()
    if a.train_updates > 1:
        names = ("plain", "reset_randomization", "plain_no_policy_tail")
        runs, episodes = {k: [] for k in names}, {k: [] for k in names}
        for rep in range(a.train_repeats):                      # alternating: the same build, the same session
            for name in names:
                rate, eps = train_rate(name, a.train_updates)
                runs[name].append(rate)
                episodes[name].append(eps)
                print("train", name, rate, eps, flush=True)
        med = {k: statistics.median(v) for k, v in runs.items()}
        result["ppo_loop"] = dict(shape="4096 envs, T = 400, 5 epochs x 50 mini-batches of 32768, HIP graphs; env-steps/s over updates 2..%d" % a.train_updates,
                                  env_steps_per_s=runs, median=med, episodes=episodes, reset_randomization_over_plain=med["reset_randomization"] / med["plain"],
                                  no_policy_tail_over_plain=med["plain_no_policy_tail"] / med["plain"],
                                  reset_randomization_over_no_policy_tail=med["reset_randomization"] / med["plain_no_policy_tail"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
