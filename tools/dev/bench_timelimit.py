#!/usr/bin/env python3
"""What time-limit bootstrapping costs: solorl_compute_returns_tl beside solorl_compute_returns (the same kernel source as before the
entry point was added) at T = 400 and 4096 / 65 536 envs, GAE and plain discounted -- device events around ONE call per timed repeat,
the median of `--repeats` repeats after `--warmup` untimed ones, one truncation per 400 steps and env (the walk recipe's own rate) --
and the kernels' registers from the built code object.

`--train-variant plain|bootstrap` instead runs ONE train() of the README recipe shape (4096 envs, T = 400, 5 epochs x 50 mini-batches of
32 768, HIP graphs) and prints its env-steps/s over the updates after the first (which holds the captures); `--root DIR` takes the
package and the launcher from another checkout (the parent commit built beside this one).  `--collect FILE...` merges the printed
lines of several such runs into `--out`.  `--variant NAME` times whatever library SOLORL_LIB names (an A/B build of the engine, e.g.
the C-ABI part compiled with -DSOLO_RETURNS_TL_BRANCH_LOAD: the non-GAE walk with its value row read under `if (tl)`) in the same way
and adds the result to `--out` under "variants" instead of replacing the file.  Nothing is gated.

    python tools/dev/bench_timelimit.py [--out profiles/r26_timelimit.json]
    python tools/dev/bench_timelimit.py --train-variant bootstrap [--train-updates 6]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def train_rate(root, variant, updates, N=4096, T=400):
    """env-steps/s of updates 2 .. `updates` of one train() run (log records: cumulative steps and their rate since the start)"""
    sys.path.insert(0, root)
    import train_ppo
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo.train import train
    argv = ["--config-file", os.path.join(root, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", str(N), "--num-steps", str(T),
            "--use-gae", "--use-linear-lr-decay", "--ppo-epoch", "5", "--mini-batch-size", "32768", "--num-env-steps", str(N * T * updates),
            "--log-interval", "1"]
    if variant == "bootstrap":
        argv += ["--bootstrap-timeouts"]
    args = train_ppo.get_ppo_args(argv)
    args.cuda = True
    config = load_yaml(args.config_file)
    config["task"] = args.task
    _, hist = train(args, config)
    t = [h["timesteps"] / h["fps"] for h in hist]                 # seconds since the loop's start at each record
    return (hist[-1]["timesteps"] - hist[0]["timesteps"]) / (t[-1] - t[0])


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join("profiles", "r26_timelimit.json"))
    p.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    p.add_argument("--steps", type=int, default=400)
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--train-variant", choices=("plain", "bootstrap"), default=None)
    p.add_argument("--train-updates", type=int, default=6)
    p.add_argument("--root", default=ROOT)
    p.add_argument("--label", default=None)
    p.add_argument("--collect", nargs="+", default=None, metavar="FILE")
    p.add_argument("--variant", default=None, metavar="NAME", help="the loaded library (SOLORL_LIB) is an A/B build: add its timings to --out under variants[NAME]")
    p.add_argument("--variant-note", default="")
    a = p.parse_args(argv)

    if a.train_variant is not None:
        rate = train_rate(os.path.abspath(a.root), a.train_variant, a.train_updates)
        print("PPO_LOOP " + json.dumps({"label": a.label or a.train_variant, "env_steps_per_s": rate}), flush=True)
        return

    if a.collect is not None:
        result = json.load(open(a.out)) if os.path.exists(a.out) else {}
        runs = {}
        for f in a.collect:
            for line in open(f):
                if line.startswith("PPO_LOOP "):
                    r = json.loads(line[len("PPO_LOOP "):])
                    runs.setdefault(r["label"], []).append(r["env_steps_per_s"])
        mean = {k: statistics.mean(v) for k, v in runs.items()}
        result["ppo_loop"] = dict(shape="4096 envs, T = 400, 5 epochs x 50 mini-batches of 32768, HIP graphs; env-steps/s over updates 2..%d; one "
                                        "process per run, alternating; the parent commit built beside this one" % a.train_updates,
                                  env_steps_per_s=runs, mean=mean)
        json.dump(result, open(a.out, "w"), indent=1, sort_keys=True)
        print(json.dumps(result["ppo_loop"], indent=1, sort_keys=True))
        return

    sys.path.insert(0, ROOT)
    import torch
    from solorl_amd import _native, devcode
    from solorl_amd.ppo.storage import RolloutStorage
    dev = torch.device("cuda:0")
    L = _native.lib()

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

    keep = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
    res = {k: v for k, v in devcode.kernel_resources(_native.LIB_PATH).items() if "returns_kernel" in k or "returns_tl_kernel" in k}
    result = dict(repeats=a.repeats, warmup=a.warmup, device=torch.cuda.get_device_name(0), steps=a.steps, sizes={},
                  kernels={k: {f: r[f] for f in keep if f in r} for k, r in res.items()},
                  note="solorl_compute_returns' kernel source is the parent commit's, unchanged; both are timed in this run")
    T = a.steps
    for N in a.sizes:
        g = torch.Generator(device=dev); g.manual_seed(0)
        st = RolloutStorage(T, N, (1,), 1, dev, bootstrap_timeouts=True)
        st.rewards.copy_(torch.randn(st.rewards.shape, device=dev, generator=g))
        st.value_preds.copy_(torch.randn(st.value_preds.shape, device=dev, generator=g))
        # an episode end per 50 steps and env, a truncation per 400: one row of timeouts, falls elsewhere
        st.masks.copy_((torch.rand(st.masks.shape, device=dev, generator=g) > 0.02).float())
        st.masks[T // 2] = 0.0
        st.timeouts[T // 2 - 1] = 1
        nv = torch.randn(N, 1, device=dev, generator=g)
        ptr = lambda x: C.c_void_p(x.data_ptr())
        stream = _native.stream(dev)
        r = {}
        for name, gae in (("gae", 1), ("discounted", 0)):
            plain = lambda: _native.check(L.solorl_compute_returns(ptr(st.rewards), ptr(st.value_preds), ptr(st.masks), ptr(nv), ptr(st.returns),
                                                                   T, N, gae, 0.99, 0.95, 0, stream))
            tl = lambda: _native.check(L.solorl_compute_returns_tl(ptr(st.rewards), ptr(st.value_preds), ptr(st.masks), ptr(st.timeouts), ptr(nv),
                                                                   ptr(st.returns), T, N, gae, 0.99, 0.95, 0, stream))
            # interleaved twice, so that a drift of the clocks shows as a spread between the two passes and not as a ratio
            a1, b1, a2, b2 = timed(plain), timed(tl), timed(plain), timed(tl)
            r[name] = dict(compute_returns=[a1, a2], compute_returns_tl=[b1, b2],
                           tl_over_plain=(b1["median_ms"] + b2["median_ms"]) / (a1["median_ms"] + a2["median_ms"]),
                           bytes_per_sample=dict(compute_returns=16 if gae else 12, compute_returns_tl=17 if gae else 16))
        result["sizes"][str(N)] = r
        del st
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.variant is not None:                                  # an A/B build beside the product's figures, which stay
        whole = json.load(open(a.out)) if os.path.exists(a.out) else {}
        whole.setdefault("variants", {})[a.variant] = dict(note=a.variant_note, lib=os.path.basename(_native.LIB_PATH), kernels=result["kernels"],
                                                           sizes=result["sizes"])
        result = whole
    json.dump(result, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(result, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
