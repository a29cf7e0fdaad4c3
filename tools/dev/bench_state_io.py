#!/usr/bin/env python3
"""What the batched state calls cost beside a step: get_states, set_states(all), push and reset_masked (half of the envs) on the fp32
Solo12 walk workload at 4096 and 65 536 envs, with one solorl_step launch of the same batch and the per-env path (get_state over 128
envs, per env) from the same run.  Device events around ONE call per timed repeat (`--calls` > 1: a train of back-to-back calls,
divided by its length); the figure is the median of `--repeats` repeats after `--warmup` untimed ones.  `reset_masked_half` is the C
entry point alone (solorl_reset_masked with an observation array); `reset_masked_half_wrapper` is SoloVecEnv.reset_masked, which
refills the observation buffer first and clones it.  `push` is SoloVecEnv.push: get_states, two torch adds, set_states(vel).
Nothing is gated; writes `--out` (default profiles/r06_state_io.json).

    python tools/dev/bench_state_io.py [--out profiles/r06_state_io.json] [--sizes 4096 65536]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join("profiles", "r06_state_io.json"))
    p.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--calls", type=int, default=1)
    a = p.parse_args(argv)

    import torch
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.state import ROW_BYTES
    from solorl_amd.vec_env import SoloVecEnv
    dev = torch.device("cuda:0")

    def timed(fn):
        ms = []
        for r in range(a.warmup + a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                ms.append(e0.elapsed_time(e1) / a.calls)
        return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))

    result = dict(workload="solo12 walk fp32, num_history_stack 1", repeats=a.repeats, warmup=a.warmup, calls_per_repeat=a.calls,
                  row_bytes=ROW_BYTES, device=torch.cuda.get_device_name(0), sizes={})
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
        dv = (torch.rand(N, 3, device=dev, generator=g) * 2 - 1) * 0.1
        half = (torch.arange(N, device=dev) % 2 == 0)
        r = {}
        r["get_states"] = timed(lambda: env.get_states(out=rows))
        r["set_states_all"] = timed(lambda: env.set_states(saved))
        r["push"] = timed(lambda: env.push(dv))                 # get + two torch adds + set(vel)
        env.set_states(saved)
        r["step"] = timed(lambda: env.step_inplace(act))
        env.set_states(saved)
        import ctypes as C
        from solorl_amd import _native
        half8, obs = half.to(torch.uint8), torch.empty(N, env.obs_dim, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        r["reset_masked_half"] = timed(lambda: _native.check(env.L.solorl_reset_masked(env._h, C.c_void_p(half8.data_ptr()), C.c_void_p(obs.data_ptr()), st)))
        env.set_states(saved)
        r["reset_masked_half_wrapper"] = timed(lambda: env.reset_masked(half))
        env.set_states(saved)
        # the per-env path: one host-synchronising call per env
        torch.cuda.synchronize()
        n_env = min(128, N)
        ms = []
        for rep in range(3):
            t0 = time.perf_counter()
            for i in range(n_env):
                env.get_state(i)
            ms.append((time.perf_counter() - t0) * 1e3 / n_env)
        r["get_state_per_env"] = dict(median_ms=statistics.median(ms), envs=n_env, whole_batch_ms=statistics.median(ms) * N)
        r["bytes"] = dict(rows=N * ROW_BYTES)
        r["push_over_step"] = r["push"]["median_ms"] / r["step"]["median_ms"]
        result["sizes"][str(N)] = r
        print(N, json.dumps(r), flush=True)
        env.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
