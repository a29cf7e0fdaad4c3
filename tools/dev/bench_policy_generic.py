#!/usr/bin/env python3
"""What the width-generic policy kernels (the _w entry points, SOLORL_POLICY_GENERIC) cost and buy, three measurements in one run:

1. against the per-shape kernels at (76, 76, 12) and (76, 96, 12) -- the same calls on both families: act at 4096 and 65 536 rows, and
   stage 1, stage 2 + 3 and clip + Adam of a mini-batch of 32 768 rows of a 16 x 4096 storage; the ratio per kernel is what flipping the
   default would cost;
2. against the PyTorch path they replace at (79, 79, 12), (79, 96, 12) and (84, 104, 12): act beside Policy.act_into on the same rows, and
   GraphedPPO's captured mini-batch step (one graph replay: gradients, clip, Adam) with the switch at 1 beside the switch unset;
3. the PPO loop of the README recipe shape with --commands at one history level (a 79-wide policy): train_ppo.py's train() in this
   process (4096 envs, T = 400, 5 epochs x 50 mini-batches of 32 768, HIP graphs, `--train-updates` updates, env-steps/s over the updates
   after the first), switch off and switch on, and -- with `--parent-tree DIR`, a built checkout of the parent commit -- that tree's loop
   with the switch off in a process of its own, alternating, `--train-repeats` times each.  Every run's value is kept: the spread of a
   leg's repeats is the only noise estimate the protocol gives.

Device events around ONE call per timed repeat; a figure is the median of `--repeats` repeats after `--warmup` untimed ones.  The
kernels' registers and LDS are read from the built code object.  Nothing is gated; writes `--out` (default profiles/r27_policy_generic.json).

    python tools/dev/bench_policy_generic.py [--out profiles/r27_policy_generic.json] [--parent-tree DIR] [--train-updates 6]"""
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


def train_rate(root, generic, updates, N=4096, T=400):
    """env-steps/s of updates 2 .. `updates` of one train() run with --commands at one history level, the switch set or unset"""
    import train_ppo
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo.train import train
    argv = ["--config-file", os.path.join(root, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", str(N), "--num-steps", str(T),
            "--use-gae", "--use-linear-lr-decay", "--ppo-epoch", "5", "--mini-batch-size", "32768", "--num-env-steps", str(N * T * updates),
            "--log-interval", "1", "--commands", os.path.join(root, "configs", "commands_walk12.yaml")]
    args = train_ppo.get_ppo_args(argv)
    args.cuda = True
    config = load_yaml(args.config_file)
    config["task"] = args.task
    config["num_history_stack"] = 1
    args.commands = train_ppo.load_commands(args.commands)
    old = os.environ.pop("SOLORL_POLICY_GENERIC", None)
    if generic:
        os.environ["SOLORL_POLICY_GENERIC"] = "1"
    try:
        _, hist = train(args, config)
    finally:
        os.environ.pop("SOLORL_POLICY_GENERIC", None)
        if old is not None:
            os.environ["SOLORL_POLICY_GENERIC"] = old
    t = [h["timesteps"] / h["fps"] for h in hist]                 # seconds since the loop's start at each record
    return (hist[-1]["timesteps"] - hist[0]["timesteps"]) / (t[-1] - t[0])


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    root = _root(argv)
    sys.path.insert(0, root)
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join("profiles", "r27_policy_generic.json"))
    p.add_argument("--repeats", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--train-updates", type=int, default=6, help="updates per train() run of the PPO-loop comparison (0 = skip it)")
    p.add_argument("--train-repeats", type=int, default=2)
    p.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its loop, switch off, joins measurement 3")
    p.add_argument("--root", default=None, help="import the loop from this tree")
    p.add_argument("--loop-only", action="store_true", help="one switch-off train() run, its rate printed as JSON (the parent leg)")
    a = p.parse_args(argv)
    if a.loop_only:
        print(json.dumps({"env_steps_per_s": train_rate(root, False, a.train_updates)}), flush=True)
        return None

    import ctypes as C
    import torch
    from solorl_amd import _native, build, devcode
    from solorl_amd.ppo import Policy, RolloutStorage
    from solorl_amd.ppo import dist as D
    from solorl_amd.ppo import fused
    from solorl_amd.ppo.fused import GENERIC, TEMPLATED, ClipAdam, MiniBatchGrad, policy_act, policy_params
    from solorl_amd.ppo.graphs import GraphedPPO
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

    def policy(O, OC, A):
        torch.manual_seed(0)
        return Policy((O,), type("Box", (), {"shape": (A,)})(), None, {"hidden_size": 64}, critic_obs_dim=None if OC == O else OC).to(dev)

    def storage(O, OC, A, T, N):
        st = RolloutStorage(T, N, (O,), A, dev, **({} if OC == O else {"critic_obs_dim": OC}))
        st.obs.normal_(); st.actions.normal_(); st.rewards.normal_(); st.value_preds.normal_(); st.returns.normal_()
        st.action_log_probs.normal_().mul_(0.1).sub_(10)
        if OC != O:
            st.critic_obs.normal_()
        return st

    def act_times(pol, O, OC, A, family, n):
        obs, noise = torch.randn(n, O, device=dev), torch.randn(n, A, device=dev)
        cobs = torch.randn(n, OC, device=dev) if OC != O else None
        v, ac, lp = torch.empty(n, 1, device=dev), torch.empty(n, A, device=dev), torch.empty(n, 1, device=dev)
        if family is None:
            kw = {} if cobs is None else {"critic_inputs": cobs}
            return timed(lambda: pol.act_into(obs, v, ac, lp, noise=noise, **kw))
        P = policy_params(pol, family)
        return timed(lambda: policy_act(P, obs, noise, v, ac, lp, critic_obs=cobs))

    def stage_times(pol, O, OC, A, family, T=16, N=4096, m=32768):
        st = storage(O, OC, A, T, N)
        D.FlatGradBucket(pol.parameters())
        off = torch.zeros((), dtype=torch.long, device=dev)
        mb = MiniBatchGrad(pol, st, m, 0.1, 0.5, 0.01, True, torch.randperm(T * N, device=dev), off, torch.randn(T * N, 1, device=dev), family=family)
        ca = ClipAdam(mb, torch.tensor(1e-4, device=dev), 0.5, offset=off, offset_increment=0)
        di, s = dev.index or 0, _native.stream(dev)
        s1 = lambda: fused._call(mb.P, "solorl_ppo_grad_stage1", [C.byref(mb.B), C.byref(mb.W), di, s], {1: mb.cobs, 3: mb.cxt0})
        s2 = lambda: fused._call(mb.P, "solorl_ppo_grad_stage2", [C.byref(mb.W), mb.m, C.byref(mb.G), di, s], {1: mb.cxt0})
        return dict(stage1=timed(s1), stage2_3=timed(s2), clip_adam=timed(ca), step=timed(lambda: (mb(), ca())))

    res = {k: v for k, v in devcode.kernel_resources(build.LIB).items() if "_w_kernel" in k or "stage2_mfma" in k}
    keep = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
    result = dict(repeats=a.repeats, warmup=a.warmup, device=torch.cuda.get_device_name(0),
                  kernels={k: {f: r[f] for f in keep if f in r} for k, r in res.items()})

    # 1. the two families on the same calls
    result["generic_over_templated"] = {}
    for O, OC, A in ((76, 76, 12), (76, 96, 12)):
        r = {}
        for family in (TEMPLATED, GENERIC):
            pol = policy(O, OC, A)
            r[family] = dict(stage_times(pol, O, OC, A, family), **{"act_%d" % n: act_times(pol, O, OC, A, family, n) for n in (4096, 65536)})
        r["ratio"] = {k: r[GENERIC][k]["median_ms"] / r[TEMPLATED][k]["median_ms"] for k in r[GENERIC]}
        result["generic_over_templated"]["%d_%d_%d" % (O, OC, A)] = r
        print((O, OC, A), json.dumps(r["ratio"]), flush=True)

    # 2. the generic family beside the PyTorch path it replaces
    result["generic_over_torch"] = {}
    for O, OC, A in ((79, 79, 12), (79, 96, 12), (84, 104, 12)):
        r = {"generic": {}, "torch": {}}
        pol = policy(O, OC, A)
        for n in (4096, 65536):
            r["generic"]["act_%d" % n] = act_times(pol, O, OC, A, GENERIC, n)
            r["torch"]["act_%d" % n] = act_times(pol, O, OC, A, None, n)
        r["generic"].update(stage_times(policy(O, OC, A), O, OC, A, GENERIC))
        for name, switch in (("torch", None), ("generic", "1")):      # the captured mini-batch step, as the loop replays it
            os.environ.pop("SOLORL_POLICY_GENERIC", None)
            if switch:
                os.environ["SOLORL_POLICY_GENERIC"] = switch
            g = GraphedPPO(policy(O, OC, A), 0.1, 1, 32768, 0.5, 0.01, lr=1e-4, max_grad_norm=0.5)
            st = storage(O, OC, A, 16, 4096)
            g.update(st)                                               # builds and captures; leaves the cursor at the end
            assert g.fused_mlp == (switch is not None)

            def replay(g=g):
                g._off.zero_()
                g._g1.replay()
            r[name]["graphed_minibatch_step"] = timed(replay)
            os.environ.pop("SOLORL_POLICY_GENERIC", None)
        r["ratio"] = {k: r["generic"][k]["median_ms"] / r["torch"][k]["median_ms"] for k in r["torch"]}
        result["generic_over_torch"]["%d_%d_%d" % (O, OC, A)] = r
        print((O, OC, A), json.dumps(r["ratio"]), flush=True)

    # 3. the PPO loop with --commands at one history level
    if a.train_updates > 1:
        legs = ["switch_off", "switch_on"] + (["parent_switch_off"] if a.parent_tree else [])
        runs = {k: [] for k in legs}
        for rep in range(a.train_repeats):                          # alternating: the same session
            for name in legs:
                if name == "parent_switch_off":
                    tree = os.path.abspath(a.parent_tree)
                    env = {k: v for k, v in os.environ.items() if k not in ("SOLORL_POLICY_GENERIC", "SOLORL_LIB")}
                    out = subprocess.run([sys.executable, HERE, "--loop-only", "--root", tree, "--train-updates", str(a.train_updates)], cwd=tree, env=env,
                                         check=True, stdout=subprocess.PIPE, timeout=900).stdout.decode()
                    runs[name].append(json.loads(out.strip().splitlines()[-1])["env_steps_per_s"])
                else:
                    runs[name].append(train_rate(root, name == "switch_on", a.train_updates))
                print("train", name, runs[name][-1], flush=True)
        med = {k: statistics.median(v) for k, v in runs.items()}
        spread = {k: max(v) - min(v) for k, v in runs.items()}
        result["ppo_loop_commands_history1"] = dict(
            shape="4096 envs, T = 400, 5 epochs x 50 mini-batches of 32768, HIP graphs, --commands configs/commands_walk12.yaml, num_history_stack 1 "
                  "(a 79-wide policy); env-steps/s over updates 2..%d; %d runs per leg, alternating" % (a.train_updates, a.train_repeats),
            env_steps_per_s=runs, median=med, spread=spread, switch_on_over_off=med["switch_on"] / med["switch_off"],
            gain_exceeds_spread=min(runs["switch_on"]) - max(runs["switch_off"]) > 0 and
            med["switch_on"] - med["switch_off"] > max(spread["switch_on"], spread["switch_off"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
