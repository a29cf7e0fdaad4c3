#!/usr/bin/env python3
"""What PPO KL control costs (solorl_ppo_grad_stage1_kl, solorl_ppo_clip_adam_kl; --ppo-diagnostics, --desired-kl), in one run on one GPU:

1. at (76, 76, 12) and (76, 96, 12), a mini-batch of 32 768 rows of a 16 x 4096 storage: stage 1 with and without the diagnostics,
   clip + Adam with and without the controller, and the four launches of a mini-batch step together (stage 1, stage 2 + 3, clip + Adam);
2. the PPO loop of the README recipe shape -- train_ppo.py's train() in this process: 4096 envs, T = 400, 5 epochs x 50 mini-batches of
   32 768, --lr 1e-3, HIP graphs, `--train-updates` updates, env-steps/s over the updates after the first -- with the flags off, with
   --ppo-diagnostics and with --desired-kl 0.01, and -- with `--parent-tree DIR`, a built checkout of the parent commit -- that tree's
   loop with the flags off in a process of its own; alternating, `--train-repeats` times each.  Every run's value is kept: the spread of
   a leg's repeats is the only noise estimate the protocol gives.

Device events around ONE call per timed repeat; a figure is the median of `--repeats` repeats after `--warmup` untimed ones.  The
kernels' registers are read from the built code object.  Nothing is gated; writes `--out` (default profiles/r28_kl_control.json).
`--bench-line FILE`: a file holding bench.py's JSON line of the same session, recorded with the rest.

    python tools/dev/bench_kl_control.py [--out profiles/r28_kl_control.json] [--parent-tree DIR] [--train-updates 6]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.abspath(__file__)


def _root(argv):
    """--root DIR: the tree the loop is imported from (the parent leg runs this file on the parent's tree)"""
    if "--root" in argv:
        return os.path.abspath(argv[argv.index("--root") + 1])
    return os.path.dirname(os.path.dirname(os.path.dirname(HERE)))


def train_rate(root, flags, updates, N=4096, T=400):
    """env-steps/s of updates 2 .. `updates` of one train() run of the recipe shape with `flags` (train_ppo.py arguments) added"""
    import train_ppo
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo.train import train
    argv = ["--config-file", os.path.join(root, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", str(N), "--num-steps", str(T),
            "--use-gae", "--lr", "1e-3", "--ppo-epoch", "5", "--mini-batch-size", "32768", "--num-env-steps", str(N * T * updates),
            "--log-interval", "1"] + list(flags)
    args = train_ppo.get_ppo_args(argv)
    args.cuda = True
    config = load_yaml(args.config_file)
    config["task"] = args.task
    _, hist = train(args, config)
    t = [h["timesteps"] / h["fps"] for h in hist]                 # seconds since the loop's start at each record
    extra = {k: hist[-1][k] for k in ("approx_kl", "clip_fraction", "lr", "kl_stopped_steps") if k in hist[-1]}
    return (hist[-1]["timesteps"] - hist[0]["timesteps"]) / (t[-1] - t[0]), extra


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    root = _root(argv)
    sys.path.insert(0, root)
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join("profiles", "r28_kl_control.json"))
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--train-updates", type=int, default=6, help="updates per train() run of the PPO-loop comparison (0 = skip it)")
    p.add_argument("--train-repeats", type=int, default=2)
    p.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its loop, flags off, joins measurement 2")
    p.add_argument("--bench-line", default=None, help="a file with bench.py's JSON line, copied into the result")
    p.add_argument("--root", default=None, help="import the loop from this tree")
    p.add_argument("--loop-only", action="store_true", help="one flags-off train() run, its rate printed as JSON (the parent leg)")
    a = p.parse_args(argv)
    if a.loop_only:
        print(json.dumps({"env_steps_per_s": train_rate(root, [], a.train_updates)[0]}), flush=True)
        return None

    import ctypes as C
    import torch
    from solorl_amd import _native, build, devcode
    from solorl_amd.ppo import Policy, RolloutStorage
    from solorl_amd.ppo import dist as D
    from solorl_amd.ppo import fused
    from solorl_amd.ppo.fused import ClipAdam, MiniBatchGrad
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

    def stage_times(O, OC, A, kl, T=16, N=4096, m=32768):
        torch.manual_seed(0)
        pol = Policy((O,), type("Box", (), {"shape": (A,)})(), None, {"hidden_size": 64}, critic_obs_dim=None if OC == O else OC).to(dev)
        st = RolloutStorage(T, N, (O,), A, dev, **({} if OC == O else {"critic_obs_dim": OC}))
        st.obs.normal_(); st.actions.normal_(); st.rewards.normal_(); st.value_preds.normal_(); st.returns.normal_()
        st.action_log_probs.normal_().mul_(0.1).sub_(10)
        if OC != O:
            st.critic_obs.normal_()
        D.FlatGradBucket(pol.parameters())
        off = torch.zeros((), dtype=torch.long, device=dev)
        mb = MiniBatchGrad(pol, st, m, 0.1, 0.5, 0.01, True, torch.randperm(T * N, device=dev), off, torch.randn(T * N, 1, device=dev), diagnostics=kl)
        # (a learning rate of 0 and no bounds above it: the timed steps move nothing, whatever the controller reads)
        ca = ClipAdam(mb, torch.tensor(0.0, device=dev), 0.5, offset=off, offset_increment=0 if not kl else m,
                      **(dict(kl_control=dict(desired_kl=0.01, lr_bounds=(0.0, 0.0), log_capacity=64)) if kl else {}))
        di, s = dev.index or 0, _native.stream(dev)
        s2 = lambda: fused._call(mb.P, "solorl_ppo_grad_stage2", [C.byref(mb.W), mb.m, C.byref(mb.G), di, s], {1: mb.cxt0})

        def s1():
            off.zero_()
            if kl:
                crit = lambda t: C.c_void_p(t.data_ptr() if mb.OC else None)
                _native.check(_native.lib().solorl_ppo_grad_stage1_kl(C.byref(mb.P), C.byref(mb.B), crit(mb.cobs), C.byref(mb.W), crit(mb.cxt0),
                                                                      C.c_void_p(mb.diag.data_ptr()), 0, di, s))
            else:
                fused._call(mb.P, "solorl_ppo_grad_stage1", [C.byref(mb.B), C.byref(mb.W), di, s], {1: mb.cobs, 3: mb.cxt0})

        def step():
            off.zero_()
            mb(); ca()
        mb()
        return dict(stage1=timed(s1), stage2_3=timed(s2), clip_adam=timed(ca), step=timed(step))

    names = ("stage1_kl_kernel", "stage1_mfma_kernel", "stage1_w_kl_kernel", "stage1_w_kernel", "clip_adam_kl_kernel", "clip_adam_kernel",
             "clip_adam_w_kl_kernel", "clip_adam_w_kernel")
    res = {k: v for k, v in devcode.kernel_resources(build.LIB).items() if any(n in k for n in names)}
    keep = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")
    result = dict(repeats=a.repeats, warmup=a.warmup, device=torch.cuda.get_device_name(0),
                  kernels={k: {f: r[f] for f in keep if f in r} for k, r in res.items()})
    if a.bench_line:
        lines = [l for l in open(a.bench_line).read().splitlines() if l.strip().startswith("{")]
        result["bench_line"] = json.loads(lines[-1]) if lines else None

    # 1. the kernels with and without
    result["kernels_ms"] = {}
    for O, OC, A in ((76, 76, 12), (76, 96, 12)):
        r = {"plain": stage_times(O, OC, A, False), "kl": stage_times(O, OC, A, True)}
        r["ratio"] = {k: r["kl"][k]["median_ms"] / r["plain"][k]["median_ms"] for k in r["kl"]}
        result["kernels_ms"]["%d_%d_%d" % (O, OC, A)] = r
        print((O, OC, A), json.dumps(r["ratio"]), flush=True)

    # 2. the PPO loop of the recipe shape
    if a.train_updates > 1:
        legs = {"flags_off": [], "ppo_diagnostics": ["--ppo-diagnostics"], "desired_kl_0.01": ["--desired-kl", "0.01"]}
        order = list(legs) + (["parent_flags_off"] if a.parent_tree else [])
        runs, last = {k: [] for k in order}, {}
        for rep in range(a.train_repeats):                          # alternating: the same session
            for name in order:
                if name == "parent_flags_off":
                    tree = os.path.abspath(a.parent_tree)
                    env = {k: v for k, v in os.environ.items() if k != "SOLORL_LIB"}
                    out = subprocess.run([sys.executable, HERE, "--loop-only", "--root", tree, "--train-updates", str(a.train_updates)], cwd=tree, env=env,
                                         check=True, stdout=subprocess.PIPE, timeout=600).stdout.decode()
                    runs[name].append(json.loads(out.strip().splitlines()[-1])["env_steps_per_s"])
                else:
                    rate, extra = train_rate(root, legs[name], a.train_updates)
                    runs[name].append(rate)
                    last[name] = extra
                print("train", name, runs[name][-1], flush=True)
        med = {k: statistics.median(v) for k, v in runs.items()}
        result["ppo_loop"] = dict(
            shape="basic12.yaml walk, 4096 envs, T = 400, 5 epochs x 50 mini-batches of 32768, --lr 1e-3, HIP graphs; env-steps/s over updates "
                  "2..%d; %d runs per leg, alternating; no training run beyond these updates was made" % (a.train_updates, a.train_repeats),
            env_steps_per_s=runs, median=med, spread={k: max(v) - min(v) for k, v in runs.items()}, last_record=last,
            over_flags_off={k: med[k] / med["flags_off"] for k in med})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
