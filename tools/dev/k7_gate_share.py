"""How often would a gated K7 cone sweep have to form its friction pairs' residual entries?  (CPU only, no GPU.)

The team sweep of the step kernel tests per sweep whether a team became quiet: no row changed by more than its threshold.  A team
whose limit or normal rows already say "no" cannot be quiet, so the friction pairs' entries only matter in sweeps in which every
limit and normal row of an unfinished env stayed within its threshold.  This tool measures the share of those sweeps on the bench's
workload (Solo12 walk, random torques, the stationary fall / reset regime after the bench's burn-in): the fp64 oracle carries the envs
(resets, terminations), and every control step's four sub-steps are re-run from the oracle's state through the kernel's fp32
lane-mode row loop on the CPU (tools/dev/k7_gate_share.cpp), which has the rows, the order, the cone projection and the K7 rule of
the team sweep and reports per sweep whether a limit / normal row exceeded its threshold.

usage: python tools/dev/k7_gate_share.py [--envs 24] [--steps 150] [--burn-in 450] [--out profiles/r07_k7_gate_cpu.txt]
       [--saved 22 --extra 23]   (instruction counts of the built heaviest sweep for the break-even share: devcode.hot_path_stats / loop_stats)
       [--case solo12_stand_pd_n9 | solo12_pointgoal_n13]   (instead of the bench's workload: a case of tests/golden/make_golden_sweep_bits_quiet.py,
                                                             its config, seed, env count, actions and steps, from reset, no burn-in)"""
import argparse, ctypes as C, os, subprocess, sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from solorl_amd.config import default_config, SoloConfig, EnvState, ROBOT_SOLO12, TASK_WALK   # noqa: E402
from oracle.oracle_py import Oracle                                                          # noqa: E402


def shim():
    so = os.path.join(HERE, "libk7_gate_share.so")
    srcs = [os.path.join(HERE, "k7_gate_share.cpp"), os.path.join(ROOT, "tests/host/host_shim.hpp"), os.path.join(ROOT, "solorl_amd/csrc/dynamics.hpp"),
            os.path.join(ROOT, "solorl_amd/csrc/spatial.hpp"), os.path.join(ROOT, "include/solorl_model_data.h"), os.path.join(ROOT, "include/solorl.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "tests/host"), "-o", so, srcs[0]])
    L = C.CDLL(so)
    L.k7_substep.argtypes = [C.POINTER(EnvState), C.POINTER(SoloConfig)] + [C.POINTER(C.c_int)] * 3 + [C.POINTER(C.c_uint64)]
    L.k7_substep.restype = None
    return L


def clone(s):
    d = EnvState()
    C.memmove(C.byref(d), C.byref(s), C.sizeof(EnvState))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=24)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--burn-in", type=int, default=450)       # bench.py: episode_length + 50, to the stationary fall / reset regime
    ap.add_argument("--saved", type=int, default=22)
    ap.add_argument("--extra", type=int, default=23)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None)
    a = ap.parse_args()
    L = shim()
    if a.case:
        import importlib.util
        spec = importlib.util.spec_from_file_location("quiet", os.path.join(ROOT, "tests", "golden", "make_golden_sweep_bits_quiet.py"))
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        cfg, acts = gen.case_inputs(a.case)
        acts = acts.astype(np.float64)
        a.envs, a.steps, a.burn_in = acts.shape[1], acts.shape[0], 0
        workload = "case %s of tests/golden/make_golden_sweep_bits_quiet.py" % a.case
        o = Oracle(cfg, a.envs, seed=gen.SEED)
    else:
        cfg = default_config(ROBOT_SOLO12, TASK_WALK)
        cfg.num_history_stack = 1
        workload = "Solo12 walk, random torques"
        o = Oracle(cfg, a.envs, seed=1)
        acts = np.random.default_rng(1234).uniform(-1, 1, size=(64, a.envs, 12))
    N = a.envs
    o.reset()
    pd = cfg.control != 0
    resets = 0
    solves = []          # (env, control step, nc, nlim, sweeps, quiet_ln bits)
    for t in range(a.burn_in + a.steps):
        act = acts[t % len(acts)]
        if t >= a.burn_in:
            for e in range(N):
                h = clone(o.get_state(e))
                tau0 = [0.0] * 12
                for ss in range(cfg.frame_skip):
                    for j in range(12):          # the torque is computed once per control step and acts in the first sub-step only unless hold_torque
                        if ss == 0:
                            u = float(np.clip(np.float32(act[e, j]), -1, 1))
                            tau0[j] = float(np.clip(cfg.kp * (u * 10 - h.q[j]) - cfg.kd * h.qd[j], -cfg.max_torque, cfg.max_torque)) if pd else u * cfg.max_torque
                        h.tau[j] = tau0[j] if (ss == 0 or cfg.hold_torque) else 0.0
                    nc, nl, sw, q = C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
                    L.k7_substep(C.byref(h), C.byref(cfg), C.byref(nc), C.byref(nl), C.byref(sw), C.byref(q))
                    solves.append((e, t, ss, nc.value, nl.value, sw.value, q.value))
        _, _, done, _ = o.step(act)
        resets += int(done.sum())
    S = np.array([s[:6] for s in solves], dtype=np.int64)
    Q = [s[6] for s in solves]
    nc = S[:, 3]
    sw = np.where(S[:, 3] + S[:, 4] > 0, S[:, 5], 0)     # (a solve without rows sweeps nothing on the GPU: not counted)
    quiet = np.array([bin(q).count("1") for q in Q])

    def share(m):
        return (quiet[m].sum() / max(1, sw[m].sum()), int(sw[m].sum()), int(m.sum()))

    lines = []
    P = lines.append
    P("K7 gate, CPU evidence: sweeps of an unfinished env in which no limit / normal row exceeded its threshold (the sweeps in which a gated")
    P("team sweep forms the friction pairs' entries), fp32 lane-mode row loop through the host shim, %s" % workload)
    P("%d envs x %d control steps x %d sub-steps after a burn-in of %d control steps (resets during the whole run: %d)" % (N, a.steps, cfg.frame_skip, a.burn_in, resets))
    P("solves %d, with rows %d, sweeps %d; contacts per solve: mean %.2f, max %d; sweeps per solve with rows: mean %.1f, share at 50: %.3f"
      % (len(sw), int((sw > 0).sum()), int(sw.sum()), nc.mean(), nc.max(), sw[sw > 0].mean(), (sw == 50).mean()))
    P("")
    P("%-44s %10s %10s %8s" % ("(env, sweep) pairs of unfinished envs", "share", "sweeps", "solves"))
    for name, m in (("overall", sw > 0), ("solves with >= 5 contacts", (sw > 0) & (nc >= 5)), ("solves that ran all 50 sweeps", sw == 50),
                    ("solves with >= 5 contacts, all 50 sweeps", (sw == 50) & (nc >= 5))):
        s_, n_, k_ = share(m)
        P("%-44s %10.4f %10d %8d" % (name, s_, n_, k_))
    # wavefront level: four envs sweep together, the wave sweeps until its last env is finished and enters the cold block when ANY
    # unfinished env of the four has quiet limit / normal rows.  Envs 4w..4w+3 of the same (control step, sub-step) form a wave here.
    ws = wq = ws5 = wq5 = 0
    per = {}
    for (e, t, ss, nc_, nl_, _), sw_, q in zip(S.tolist(), sw.tolist(), Q):
        per.setdefault((e // 4, t, ss), []).append((nc_, sw_, q if sw_ else 0))
    for grp in per.values():
        n_sw = max(g[1] for g in grp)
        ent = 0
        for g in grp:
            ent |= g[2]                      # (an env's bits stop at its last sweep: finished envs do not enter)
        k = bin(ent).count("1")
        ws += n_sw; wq += k
        if max(g[0] for g in grp) >= 5:
            ws5 += n_sw; wq5 += k
    P("")
    P("wavefront level (4 envs per wave, %d waves per sub-step): share of a wave's sweeps that enter the cold block" % ((N + 3) // 4))
    P("%-44s %10.4f %10d" % ("all waves", wq / max(1, ws), ws))
    P("%-44s %10.4f %10d" % ("waves with >= 5 contacts in some env", wq5 / max(1, ws5), ws5))
    be = a.saved / a.extra
    s5 = share((sw > 0) & (nc >= 5))[0]
    P("")
    P("break-even: a gated sweep issues %d instructions less, a sweep that enters the cold block %d more -> share %.3f; half of it %.3f"
      % (a.saved, a.extra, be, be / 2))
    P("measured share for the solves with >= 5 contacts: %.4f -> %s" % (s5, "GO (below half the break-even)" if s5 < be / 2 else "STOP (not below half the break-even)"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
