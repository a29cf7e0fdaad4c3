#!/usr/bin/env python3
"""What solorl_dynamics costs: one call over 4096 and 65 536 state rows of the fp32 Solo12 walk workload, beside get_states,
solorl_kinematics (the same memory shape, three quarters of the output bytes) and one eagerly launched solorl_step of the same batch,
all from the same run.  Device events around ONE call per timed repeat; the figure is the median of `--repeats` repeats after
`--warmup` untimed ones.  `get_dynamics` is SoloVecEnv.get_dynamics: get_states into the engine-owned rows, then the call.  Nothing
is gated; writes `--out` (default profiles/r14_dyn.json).

    python tools/dev/bench_dyn.py [--out profiles/r14_dyn.json] [--sizes 4096 65536]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join("profiles", "r14_dyn.json"))
    p.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    a = p.parse_args(argv)

    import torch
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.dyn_tensors import dynamics, DynBatch, ROW_BYTES as DYN_ROW_BYTES, ENVS_PER_WORKGROUP
    from solorl_amd.kinematics import kinematics, KinBatch
    from solorl_amd.state import ROW_BYTES
    from solorl_amd.vec_env import SoloVecEnv
    dev = torch.device("cuda:0")
    IN_BYTES = 37 * 8                                           # pos .. qd of a state row

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

    result = dict(workload="solo12 walk fp32, num_history_stack 1", repeats=a.repeats, warmup=a.warmup, state_row_bytes=ROW_BYTES,
                  dyn_row_bytes=DYN_ROW_BYTES, state_bytes_read_per_row=IN_BYTES, envs_per_workgroup=ENVS_PER_WORKGROUP,
                  device=torch.cuda.get_device_name(0), sizes={})
    for N in a.sizes:
        cfg = default_config(ROBOT_SOLO12, TASK_WALK); cfg.num_history_stack = 1
        env = SoloVecEnv(cfg, N, device=dev, seed=1)
        env.reset()
        g = torch.Generator(device=dev); g.manual_seed(0)
        act = (torch.rand(N, env.act_dim, device=dev, generator=g) * 2 - 1) * 0.5
        for _ in range(20):                                     # contacts: a state as a rollout has it
            env.step_inplace(act)
        rows = env.get_states()
        dyn, kin = DynBatch(N, dev), KinBatch(N, dev)
        half = (torch.arange(N, device=dev) % 2 == 0)
        r = {}
        r["get_states"] = timed(lambda: env.get_states(out=rows))
        r["kinematics"] = timed(lambda: kinematics(env.cfg, rows, out=kin))
        r["dynamics"] = timed(lambda: dynamics(env.cfg, rows, out=dyn))
        r["dynamics_half_masked"] = timed(lambda: dynamics(env.cfg, rows, mask=half, out=dyn))
        r["get_dynamics"] = timed(lambda: env.get_dynamics(out=dyn))
        r["step"] = timed(lambda: env.step_inplace(act))
        r["bytes"] = dict(get_states_rows_written=N * ROW_BYTES, dynamics=N * (IN_BYTES + DYN_ROW_BYTES))
        r["dynamics_over_get_states"] = r["dynamics"]["median_ms"] / r["get_states"]["median_ms"]
        r["dynamics_over_kinematics"] = r["dynamics"]["median_ms"] / r["kinematics"]["median_ms"]
        r["dynamics_over_step"] = r["dynamics"]["median_ms"] / r["step"]["median_ms"]
        r["dynamics_GBps"] = r["bytes"]["dynamics"] / (r["dynamics"]["median_ms"] * 1e6)
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
