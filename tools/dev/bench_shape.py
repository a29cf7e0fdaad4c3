#!/usr/bin/env python3
"""What solorl_shape_reward costs: one call over 4096 and 65 536 state rows of the fp32 Solo12 walk workload, alone and behind
get_states (what a step with shaping pays), beside one eagerly launched solorl_step of the same batch and beside the same sixteen terms
written in eager torch ops on get_states + get_kinematics -- the path that existed before the kernel -- all from the same run.
Device events around ONE call per timed repeat; the figure is the median of `--repeats` repeats after `--warmup` untimed ones.
`--train-pair N` adds a PPO-loop throughput pair (graphed rollout of T steps + the PPO update, with and without shaping, alternating).
Nothing is gated; writes `--out` (default profiles/r19_shape.json).

    python tools/dev/bench_shape.py [--out profiles/r19_shape.json] [--sizes 4096 65536]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

WEIGHTS = {"lin_vel_z": -2.0, "ang_vel_xy": -0.05, "orientation": -1.0, "base_height": -10.0, "torques": -1e-4, "joint_vel": -1e-3,
           "joint_acc": -2.5e-7, "action_rate": -0.01, "power": -1e-3, "foot_slip": -0.1, "foot_clearance": -1.0, "foot_force": -0.01,
           "feet_air_time": 1.0, "collision": -1.0, "tracking_lin_vel": 1.0, "tracking_yaw_rate": 0.5}


def torch_terms(torch, cfg, P, sb, kin, actions, done, mem, reward, terms, ep):
    """The term table of include/solorl.h in eager torch ops on a StateBatch and a KinBatch (fp64), with the same memory updates."""
    from solorl_amd.kinematics import FOOT_PRIMS
    dtc = cfg.sim_dt * cfg.frame_skip
    x, y, z, w = sb.quat.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
    vb = torch.einsum("nij,ni->nj", R, sb.lin_vel)
    wb = torch.einsum("nij,ni->nj", R, sb.ang_vel)
    gb = -R[:, 2, :]
    valid = (mem.valid != 0).double()
    a = actions.double()
    cm = sb.contact_mask
    cf = ((cm.unsqueeze(1) >> torch.tensor(FOOT_PRIMS, device=cm.device, dtype=torch.int32)) & 1).double()
    u, p, F = kin.foot_vel, kin.foot_pos, kin.foot_force
    sp2 = u[:, :, 0] ** 2 + u[:, :, 1] ** 2
    air = mem.air_time + dtc
    prev = ((mem.prev_contact.unsqueeze(1) >> torch.arange(4, device=cm.device, dtype=torch.int32)) & 1).double()
    first = valid.unsqueeze(1) * cf * (1 - prev)
    others = torch.tensor([b for b in range(24) if b not in FOOT_PRIMS], device=cm.device, dtype=torch.int32)
    t = torch.stack([
        vb[:, 2] ** 2, wb[:, 0] ** 2 + wb[:, 1] ** 2, gb[:, 0] ** 2 + gb[:, 1] ** 2, (sb.pos[:, 2] - P.base_height_target) ** 2,
        (sb.tau ** 2).sum(1), (sb.qd ** 2).sum(1), valid * (((sb.qd - mem.prev_qd) / dtc) ** 2).sum(1), valid * ((a - mem.prev_action) ** 2).sum(1),
        (sb.tau * sb.qd).abs().sum(1), (cf * sp2).sum(1), ((1 - cf) * (p[:, :, 2] - P.foot_clearance_target) ** 2 * sp2.sqrt()).sum(1),
        (F - P.foot_force_max).clamp_min(0).sum(1), (first * (air - P.air_time_target)).sum(1),
        ((cm.unsqueeze(1) >> others) & 1).sum(1).double(),
        torch.exp(-((vb[:, 0] - P.cmd_lin_vel[0]) ** 2 + (vb[:, 1] - P.cmd_lin_vel[1]) ** 2) / P.tracking_sigma),
        torch.exp(-(wb[:, 2] - P.cmd_yaw_rate) ** 2 / P.tracking_sigma)], 1)
    wts = torch.tensor(list(P.weight), dtype=torch.float64, device=cm.device)
    live = (done == 0)
    lv = live.double().unsqueeze(1)
    wt = t * wts
    terms.copy_(t * lv)
    reward.copy_(torch.where(live, (reward.double() + wt.sum(1)).float(), reward))
    ep[0] += 1 - lv[:, 0]
    ep[1:] += (mem.ep_sum * (1 - lv)).t()
    mem.ep_sum.copy_((mem.ep_sum + wt) * lv)
    mem.air_time.copy_(air * (1 - cf) * lv)
    mem.prev_action.copy_(torch.where(live.unsqueeze(1), a, mem.prev_action))
    mem.prev_qd.copy_(torch.where(live.unsqueeze(1), sb.qd, mem.prev_qd))
    mem.prev_contact.copy_(torch.where(live, (cf.int() << torch.arange(4, device=cm.device, dtype=torch.int32)).sum(1).int(), torch.zeros_like(mem.prev_contact)))
    mem.valid.copy_(live.int())


def train_pair(N, T, updates, pairs):
    """env-steps/s of the PPO loop (solorl_amd.ppo.train.train: graphed rollout of T steps + 5 epochs of mini-batches of 32 768) with and
    without shaping, alternating; the figure of a run is its last log line's, which counts from the start (graph capture included)"""
    import types
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo.train import train
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    config = load_yaml(os.path.join(root, "configs", "basic12.yaml"))
    config["task"] = "walk"
    out = {"plain": [], "shaped": []}
    for _ in range(pairs):
        for name in ("plain", "shaped"):
            args = types.SimpleNamespace(
                num_agents=N, hidden_size=64, cuda=True, gamma=0.99, tau=0.95, clip_param=0.1, ppo_epoch=5, mini_batch_size=32768, lr=2.5e-4,
                l2_coef=0.0, value_loss_coef=0.5, entropy_coef=0.01, max_grad_norm=0.5, use_linear_lr_decay=False, use_gae=True,
                num_env_steps=N * T * updates, seed=1, curriculum_schedule=0, log_interval=1, logdir=None, base_checkpoint=None, save_interval=1,
                num_steps=T, reward_shaping=dict(weights=WEIGHTS) if name == "shaped" else None)
            _, hist = train(args, config)
            out[name].append(hist[-1]["fps"])
    return dict(envs=N, steps=T, updates=updates, pairs=pairs, env_steps_per_s=out,
                shaped_over_plain=statistics.mean(out["shaped"]) / statistics.mean(out["plain"]))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join("profiles", "r19_shape.json"))
    p.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--train-pair", type=int, default=0, metavar="N", help="also time the PPO loop on N envs with and without shaping (0 = skip)")
    p.add_argument("--train-steps", type=int, default=400)
    p.add_argument("--train-updates", type=int, default=4)
    a = p.parse_args(argv)

    import torch
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.kinematics import KinBatch
    from solorl_amd.shaping import ENVS_PER_WORKGROUP, EP_FIELDS, ROW_BYTES, SHAPE_TERMS, ShapeMem, make_params, shape_reward
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

    P = make_params(WEIGHTS)
    result = dict(workload="solo12 walk fp32, num_history_stack 1", repeats=a.repeats, warmup=a.warmup, mem_row_bytes=ROW_BYTES,
                  state_bytes_read_per_row=54 * 8, envs_per_workgroup=ENVS_PER_WORKGROUP, device=torch.cuda.get_device_name(0), sizes={})
    for N in a.sizes:
        cfg = default_config(ROBOT_SOLO12, TASK_WALK); cfg.num_history_stack = 1
        env = SoloVecEnv(cfg, N, device=dev, seed=1)
        env.reset()
        g = torch.Generator(device=dev); g.manual_seed(0)
        act = (torch.rand(N, env.act_dim, device=dev, generator=g) * 2 - 1) * 0.5
        for _ in range(20):                                     # contacts: a state as a rollout has it
            o, rew, done, _ = env.step_inplace(act)
        rows, kin, mem = env.get_states(), KinBatch(N, dev), ShapeMem(N, dev)
        terms = torch.zeros(N, SHAPE_TERMS, dtype=torch.float64, device=dev)
        ep = torch.zeros(EP_FIELDS, N, dtype=torch.float64, device=dev)
        reward = rew.clone()

        def kernel():
            shape_reward(env.cfg, P, rows, act, done, mem, reward, terms_out=terms, ep_out=ep)

        def with_states():
            env.get_states(out=rows)
            kernel()

        def torch_path():
            env.get_states(out=rows)
            env.get_kinematics(states=rows, out=kin)
            torch_terms(torch, env.cfg, P, rows, kin, act, done, mem, reward, terms, ep)

        # the two formulations agree on this batch before either is timed
        m2, t2, e2, r2 = ShapeMem(N, dev), terms.clone(), ep.clone(), rew.clone()
        shape_reward(env.cfg, P, rows, act, done, mem, reward, terms_out=terms, ep_out=ep)
        env.get_kinematics(states=rows, out=kin)
        torch_terms(torch, env.cfg, P, rows, kin, act, done, m2, r2, t2, e2)
        agree = float((terms - t2).abs().max() / terms.abs().max().clamp_min(1.0))
        r = {"torch_terms_max_rel_diff": agree}
        r["get_states"] = timed(lambda: env.get_states(out=rows))
        r["shape_reward"] = timed(kernel)
        r["get_states_shape_reward"] = timed(with_states)
        r["torch_get_states_get_kinematics_terms"] = timed(torch_path)
        r["step"] = timed(lambda: env.step_inplace(act))
        env.set_reward_shaping(WEIGHTS)
        r["step_with_shaping"] = timed(lambda: env.step_inplace(act))
        r["shape_reward_over_step"] = r["shape_reward"]["median_ms"] / r["step"]["median_ms"]
        r["get_states_shape_reward_over_step"] = r["get_states_shape_reward"]["median_ms"] / r["step"]["median_ms"]
        r["torch_over_kernel_path"] = r["torch_get_states_get_kinematics_terms"]["median_ms"] / r["get_states_shape_reward"]["median_ms"]
        result["sizes"][str(N)] = r
        print(N, json.dumps(r), flush=True)
        env.close()
    if a.train_pair:
        result["ppo_loop_pair_one_run"] = train_pair(a.train_pair, a.train_steps, a.train_updates, 2)
        print(json.dumps(result["ppo_loop_pair_one_run"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
