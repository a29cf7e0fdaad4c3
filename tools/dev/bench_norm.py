#!/usr/bin/env python3
"""What the running normalisation costs beside a step: solorl_normalize_obs(update = 1) for one row of [N][42] observations and
solorl_normalize_rewards(update = 1) for 400 rows of [N] rewards, at 4096 and 65 536 envs, against the same arithmetic written with
torch ops in the same process (fp64 statistics, the reference's formulas row after row: agents/running_mean_std.py:18-39, :96-116) and
beside one eager solorl_step launch of the fp32 Solo12 walk workload (num_history_stack 1) at the same batch size.  The observation
width 42 is the Solo12 single-frame observation with a goal (the kernels take any width; the data here is synthetic).  Device events
around one call per timed repeat; the figure is the median of `--repeats` repeats after `--warmup` untimed ones.  Nothing is gated;
writes `--out` (default profiles/r11_norm.json).

    python tools/dev/bench_norm.py [--out profiles/r11_norm.json] [--sizes 4096 65536]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join("profiles", "r11_norm.json"))
    p.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--obs-dim", type=int, default=42)
    p.add_argument("--rows", type=int, default=400)
    a = p.parse_args(argv)

    import torch
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.normalize import VecNormalizer
    from solorl_amd.vec_env import SoloVecEnv
    dev = torch.device("cuda:0")
    D, T, gamma, clip, eps = a.obs_dim, a.rows, 0.99, 10.0, 1e-8

    def timed(fn, setup=None):
        ms = []
        for r in range(a.warmup + a.repeats):
            if setup is not None:
                setup()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))

    def merge(st, bm, bv, n):               # running_mean_std.py:28-39 on (mean, var, count) device tensors, in place
        mean, var, count = st
        delta, tot = bm - mean, count + n
        mean += delta * n / tot
        var.copy_((var * count + bv * n + delta.square() * count * n / tot) / tot)
        count.copy_(tot)

    result = dict(obs_dim=D, reward_rows=T, repeats=a.repeats, warmup=a.warmup, device=torch.cuda.get_device_name(0),
                  step_workload="solo12 walk fp32, num_history_stack 1", sizes={})
    for N in a.sizes:
        g = torch.Generator(device=dev); g.manual_seed(0)
        x = torch.randn(N, D, device=dev, generator=g) * torch.logspace(-2, 1.5, D, device=dev) + 1.0
        rew0 = torch.randn(T, N, device=dev, generator=g) * 0.5 + 0.3
        done = (torch.rand(T, N, device=dev, generator=g) < 0.0025).to(torch.uint8)
        vn = VecNormalizer(N, D, dev, True, True, clip, clip, gamma, eps)
        vn.scratch(T, 1)
        out, rew = torch.empty_like(x), rew0.clone()
        r = {}
        r["normalize_obs_1row"] = timed(lambda: vn.obs(x, 1, True, out=out))
        r["normalize_obs_1row_frozen"] = timed(lambda: vn.obs(x, 1, False, out=out))
        r["normalize_rewards_%drows" % T] = timed(lambda: vn.rewards(rew, done, T, True), setup=lambda: rew.copy_(rew0))
        r["normalize_rewards_%drows_frozen" % T] = timed(lambda: vn.rewards(rew, done, T, False), setup=lambda: rew.copy_(rew0))

        # the same arithmetic with torch ops
        ob = [torch.zeros(D, dtype=torch.float64, device=dev), torch.ones(D, dtype=torch.float64, device=dev), torch.full((), 1e-4, dtype=torch.float64, device=dev)]
        rt = [torch.zeros((), dtype=torch.float64, device=dev), torch.ones((), dtype=torch.float64, device=dev), torch.full((), 1e-4, dtype=torch.float64, device=dev)]
        ret = torch.zeros(N, dtype=torch.float64, device=dev)
        dmask = done.bool()

        def torch_obs():
            x64 = x.double()
            merge(ob, x64.mean(0), x64.var(0, unbiased=False), N)
            out.copy_(((x64 - ob[0]) / (ob[1] + eps).sqrt()).clamp_(-clip, clip))

        def torch_rew():
            nonlocal ret
            for t in range(T):
                ret = ret * gamma + rew[t]
                merge(rt, ret.mean(), ret.var(unbiased=False), N)
                rew[t] = (rew[t] / (rt[1] + eps).sqrt()).clamp_(-clip, clip)
                ret.masked_fill_(dmask[t], 0.0)
        r["torch_obs_1row"] = timed(torch_obs)
        r["torch_rewards_%drows" % T] = timed(torch_rew, setup=lambda: rew.copy_(rew0))

        cfg = default_config(ROBOT_SOLO12, TASK_WALK); cfg.num_history_stack = 1
        env = SoloVecEnv(cfg, N, device=dev, seed=1)
        env.reset()
        act = (torch.rand(N, env.act_dim, device=dev, generator=g) * 2 - 1) * 0.5
        for _ in range(20):
            env.step_inplace(act)
        r["step"] = timed(lambda: env.step_inplace(act))
        env.close()
        r["obs_over_torch"] = r["normalize_obs_1row"]["median_ms"] / r["torch_obs_1row"]["median_ms"]
        r["rewards_over_torch"] = r["normalize_rewards_%drows" % T]["median_ms"] / r["torch_rewards_%drows" % T]["median_ms"]
        r["obs_over_step"] = r["normalize_obs_1row"]["median_ms"] / r["step"]["median_ms"]
        result["sizes"][str(N)] = r
        print(N, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
