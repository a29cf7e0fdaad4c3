#!/usr/bin/env python3
"""What the privileged critic rows cost beside a step: solorl_critic_obs alone, the stage a step gains with critic_obs set (get_states +
solorl_critic_obs), one eagerly launched step of the same run, and the same words as eager torch ops on get_states + get_kinematics --
on the fp32 Solo12 walk workload at 4096 and 65 536 envs, all in one run.  Device events around ONE call per timed repeat; the figure
is the median of `--repeats` repeats after `--warmup` untimed ones.  Then the policy side: solorl_policy_act_critic (76, 96, 12) beside
solorl_policy_act (76, 12) and the two act_into on the same rows, and the mini-batch step (MiniBatchGrad + ClipAdam, 32 768 rows of a
16 x 4096 storage) of the asymmetric policy beside the symmetric one.

Then the PPO loop (`--train-updates` > 0): train_ppo.py's train() in this process, README recipe shape (4096 envs, T = 400, 5 epochs x
50 mini-batches of 32 768, HIP graphs), without the flag, with --privileged-critic, and without it under SOLORL_STEP_ACT=0 (the
policy tail given up, which the flag forces: that share of the loss is not the stage's), alternating, `--train-repeats` times each;
env-steps/s over the updates after the first one (which holds the captures).

The kernel's registers and LDS are read from the built code object.  Nothing is gated; writes `--out` (default profiles/r24_critic.json).

    python tools/dev/bench_critic.py [--out profiles/r24_critic.json] [--sizes 4096 65536] [--train-updates 6]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def train_rate(variant, updates, N=4096, T=400):
    """env-steps/s of updates 2 .. `updates` of one train() run (log records: cumulative steps and their rate since the start)"""
    import train_ppo
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo.train import train
    argv = ["--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", str(N), "--num-steps", str(T),
            "--use-gae", "--use-linear-lr-decay", "--ppo-epoch", "5", "--mini-batch-size", "32768", "--num-env-steps", str(N * T * updates),
            "--log-interval", "1"]
    if variant == "privileged_critic":
        argv += ["--privileged-critic"]
    args = train_ppo.get_ppo_args(argv)
    args.cuda = True
    config = load_yaml(args.config_file)
    config["task"] = args.task
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
    return (hist[-1]["timesteps"] - hist[0]["timesteps"]) / (t[-1] - t[0])


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join("profiles", "r24_critic.json"))
    p.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--train-updates", type=int, default=6, help="updates per train() run of the PPO-loop comparison (0 = skip it)")
    p.add_argument("--train-repeats", type=int, default=2)
    a = p.parse_args(argv)

    import torch
    from solorl_amd import build, devcode
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.critic_obs import CRITIC_PRIV, critic_obs
    from solorl_amd.ppo import Policy
    from solorl_amd.ppo.fused import policy_act, policy_params
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

    res = {k: v for k, v in devcode.kernel_resources(build.LIB).items() if "critic_rows_kernel" in k}
    keep = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
    result = dict(workload="solo12 walk fp32, num_history_stack 1", repeats=a.repeats, warmup=a.warmup, device=torch.cuda.get_device_name(0), sizes={},
                  kernels={k: {f: r[f] for f in keep if f in r} for k, r in res.items()})
    for N in a.sizes:
        cfg = default_config(ROBOT_SOLO12, TASK_WALK); cfg.num_history_stack = 1
        env = SoloVecEnv(cfg, N, device=dev, seed=1, critic_obs=True)
        env.reset()
        g = torch.Generator(device=dev); g.manual_seed(0)
        act = torch.rand(N, env.act_dim, device=dev, generator=g) * 2 - 1
        for _ in range(20):                                     # contacts, history: a state as a rollout has it
            env.step_inplace(act)
        rows = env.get_states()
        clean = env.get_observation().clone()
        E = env.engine_obs_dim
        out = torch.empty(N, E + CRITIC_PRIV, device=dev)
        scale = torch.tensor(list(env._critic.scale), dtype=torch.float64, device=dev)
        r = {}
        r["critic_obs"] = timed(lambda: critic_obs(cfg, env._critic, rows, clean, out=out))
        r["stage"] = timed(lambda: env._critic_rows(clean))      # get_states + the kernel, as behind a step
        stage = env._critic
        env._critic = None                                       # (the step launch alone)
        r["step"] = timed(lambda: env.step_inplace(act))
        env._critic = stage

        def torch_words():
            s = env.get_states(out=rows)
            kin = env.get_kinematics(states=s)
            feet = [13, 15, 17, 19]
            u = kin.prim_vel[:, feet]
            cm = s.contact_mask
            coll = torch.zeros(N, dtype=torch.float64, device=dev)
            for p_ in range(24):
                if p_ not in feet:
                    coll += ((cm >> p_) & 1).to(torch.float64)
            z = torch.zeros(N, 1, dtype=torch.float64, device=dev)
            raw = torch.cat([kin.prim_force[:, feet], kin.prim_point[:, feet, 2], (u[:, :, 0] * u[:, :, 0] + u[:, :, 1] * u[:, :, 1]).sqrt(), z, z, z,
                             s.timestep.to(torch.float64).unsqueeze(1), coll.unsqueeze(1), z, z, z], dim=1)
            torch.cat([clean, (raw * scale).to(torch.float32)], dim=1, out=out)
        r["torch_words_and_kinematics"] = timed(torch_words)
        r["stage_over_step"] = r["stage"]["median_ms"] / r["step"]["median_ms"]
        r["torch_over_stage"] = r["torch_words_and_kinematics"]["median_ms"] / r["stage"]["median_ms"]

        # the policy side: the act kernel with a critic width beside the symmetric one, and the PyTorch forms of both
        torch.manual_seed(0)
        sym = Policy((E,), env.action_space, None, {"hidden_size": 64}).to(dev)
        asym = Policy((E,), env.action_space, None, {"hidden_size": 64}, critic_obs_dim=E + CRITIC_PRIV).to(dev)
        P = policy_params(sym)
        noise = torch.randn(N, env.act_dim, device=dev)
        v, ac, lp = torch.empty(N, 1, device=dev), torch.empty(N, env.act_dim, device=dev), torch.empty(N, 1, device=dev)
        PA = policy_params(asym)
        r["policy_act_kernel_symmetric"] = timed(lambda: policy_act(P, clean, noise, v, ac, lp))
        r["policy_act_critic_kernel"] = timed(lambda: policy_act(PA, clean, noise, v, ac, lp, critic_obs=out))
        r["act_into_asymmetric"] = timed(lambda: asym.act_into(clean, v, ac, lp, noise=noise, critic_inputs=out))
        r["act_into_symmetric"] = timed(lambda: sym.act_into(clean, v, ac, lp, noise=noise))
        result["sizes"][str(N)] = r
        print(N, json.dumps(r), flush=True)
        env.close()
    # the mini-batch step at the recipe's size: gradients (three launches) + clip and Adam (one), symmetric (76, 12) and asymmetric (76, 96, 12)
    from solorl_amd.ppo import RolloutStorage
    from solorl_amd.ppo import dist as D
    from solorl_amd.ppo.fused import ClipAdam, MiniBatchGrad
    T, N, m = 16, 4096, 32768
    result["minibatch_step"] = {}
    for name, oc in (("symmetric_76_12", None), ("asymmetric_76_96_12", 96)):
        torch.manual_seed(0)
        pol = Policy((76,), type("Box", (), {"shape": (12,)})(), None, {"hidden_size": 64}, critic_obs_dim=oc).to(dev)
        st = RolloutStorage(T, N, (76,), 12, dev, critic_obs_dim=oc)
        st.obs.normal_(); st.actions.normal_(); st.value_preds.normal_(); st.returns.normal_(); st.action_log_probs.normal_().mul_(0.1).sub_(10)
        if oc:
            st.critic_obs.normal_()
        D.FlatGradBucket(pol.parameters())
        off = torch.zeros((), dtype=torch.long, device=dev)
        mb = MiniBatchGrad(pol, st, m, 0.1, 0.5, 0.01, True, torch.randperm(T * N, device=dev), off, torch.randn(T * N, 1, device=dev))
        ca = ClipAdam(mb, torch.tensor(1e-4, device=dev), 0.5, offset=off, offset_increment=0)
        result["minibatch_step"][name] = dict(gradients=timed(mb), clip_adam=timed(ca), step=timed(lambda: (mb(), ca())))
        print(name, json.dumps(result["minibatch_step"][name]), flush=True)
    if a.train_updates > 1:
        names = ("plain", "privileged_critic", "plain_no_policy_tail")
        runs = {k: [] for k in names}
        for rep in range(a.train_repeats):                      # alternating: the same build, the same session
            for name in names:
                runs[name].append(train_rate(name, a.train_updates))
                print("train", name, runs[name][-1], flush=True)
        med = {k: statistics.median(v) for k, v in runs.items()}
        result["ppo_loop"] = dict(shape="4096 envs, T = 400, 5 epochs x 50 mini-batches of 32768, HIP graphs; env-steps/s over updates 2..%d" % a.train_updates,
                                  env_steps_per_s=runs, median=med, privileged_critic_over_plain=med["privileged_critic"] / med["plain"],
                                  no_policy_tail_over_plain=med["plain_no_policy_tail"] / med["plain"],
                                  privileged_critic_over_no_policy_tail=med["privileged_critic"] / med["plain_no_policy_tail"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
