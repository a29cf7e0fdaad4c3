#!/usr/bin/env python3
"""Golden vectors for the running normalisation, produced by IMPORTING the reference's agents/running_mean_std.py by file path
(numpy only) and driving its real VecNormalize over a stub venv that replays recorded observations, rewards and done flags.  Only
inputs/outputs are written (tests/golden/norm_golden.npz); no reference source or bytecode is copied.  Needs the reference checkout
beside the repository's build container; the tests read the .npz only.

Per case (suffix _n5, _n67; D = 42, T = 24 steps):
  obs_raw [T+1][n][D] f32 (row 0 = the reset's), rew_raw [T][n] f32, done [T][n] bool        what the stub venv returns
  obs_ref [T+1][n][D] f32, rew_ref [T][n] f64                                                what VecNormalize returns
  ob_mean / ob_var [T+1][D], ob_count [T+1], rt_mean / rt_var / rt_count [T], ret [T][n]     its statistics and accumulator after every call
  ref_vs_f64_obs, ref_vs_f64_rew                                                             max |reference - tests/norm_ref.py| over the outputs
The reference keeps the observation statistics in float32 (its observations are float32), the return statistics in float64."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get("SOLORL_REFERENCE", "/root/reference")
D, T = 42, 24


def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


class StubVenv:
    def __init__(self, obs, rew, done):
        self.obs, self.rew, self.done, self.t = obs, rew, done, 0
        self.nenvs = obs.shape[1]
        self.observation_space = types.SimpleNamespace(shape=obs.shape[2:])
        self.action_space = types.SimpleNamespace(shape=(12,))

    def reset(self):
        return self.obs[0]

    def step(self, actions):
        t = self.t
        self.t += 1
        return self.obs[t + 1], self.rew[t], self.done[t], [{} for _ in range(self.nenvs)]


def inputs(n, rng):
    scale = np.geomspace(1e-2, 30.0, D)                       # column scales 1e-2 .. 30
    mean = rng.uniform(-3.0, 3.0, D) * scale                  # non-zero means
    obs = (mean + scale * rng.standard_normal((T + 1, n, D))).astype(np.float32)
    # a few values pushed beyond the clip (10 sigma).  An outlier x among `count` samples raises the variance by about x^2 / count, so
    # its own normalised value cannot exceed sqrt(count): they come late (count >= 5 * 23) and are far out
    for _ in range(6):
        t, e, d = rng.integers(T - 2, T + 1), rng.integers(n), rng.integers(D)
        obs[t, e, d] = np.float32(mean[d] + scale[d] * rng.choice([-1000.0, 1000.0]))
    rew = (0.3 + 0.5 * rng.standard_normal((T, n))).astype(np.float32)
    rew[T - 1, rng.integers(n)] = np.float32(-1000.0)
    done = rng.random((T, n)) < 0.2
    return obs, rew, done


def main():
    import norm_ref
    rms = load("ref_running_mean_std", "agents/running_mean_std.py")
    rng = np.random.default_rng(20261019)
    out = {}
    for n in (5, 67):
        obs, rew, done = inputs(n, rng)
        vn = rms.VecNormalize(StubVenv(obs, rew, done), ob=True, ret=True, clipob=10., cliprew=10., gamma=0.99, epsilon=1e-8)
        f64 = norm_ref.NormRef(n, D, 10., 10., 0.99, 1e-8)
        rec = dict(obs_ref=[], rew_ref=[], ob_mean=[], ob_var=[], ob_count=[], rt_mean=[], rt_var=[], rt_count=[], ret=[])
        dobs = drew = 0.0

        def ob_state(o, o64):
            rec["obs_ref"].append(np.asarray(o)); rec["ob_mean"].append(np.asarray(vn.ob_rms.mean)); rec["ob_var"].append(np.asarray(vn.ob_rms.var))
            rec["ob_count"].append(vn.ob_rms.count)
            return float(np.abs(np.asarray(o, np.float64) - o64).max())

        dobs = max(dobs, ob_state(vn.reset(), f64.obs(obs[0])))
        f64.reset()
        for t in range(T):
            o, r, _, _ = vn.step(None)
            r64 = f64.rewards(rew[t], done[t])
            dobs = max(dobs, ob_state(o, f64.obs(obs[t + 1])))
            drew = max(drew, float(np.abs(np.asarray(r, np.float64) - r64).max()))
            rec["rew_ref"].append(np.asarray(r, np.float64)); rec["rt_mean"].append(float(vn.ret_rms.mean)); rec["rt_var"].append(float(vn.ret_rms.var))
            rec["rt_count"].append(vn.ret_rms.count); rec["ret"].append(np.array(vn.ret, np.float64))
        assert (np.abs(np.stack(rec["obs_ref"])) == 10.0).sum() >= 3 and (np.abs(np.stack(rec["rew_ref"])) == 10.0).sum() >= 1
        sfx = "_n%d" % n
        out.update({"obs_raw" + sfx: obs, "rew_raw" + sfx: rew, "done" + sfx: done, "ref_vs_f64_obs" + sfx: np.float64(dobs),
                    "ref_vs_f64_rew" + sfx: np.float64(drew)})
        out.update({k + sfx: np.stack(v) if np.ndim(v[0]) else np.asarray(v) for k, v in rec.items()})
        print("n = %d: ref_vs_f64_obs %.3e ref_vs_f64_rew %.3e" % (n, dobs, drew))
    path = os.path.join(HERE, "norm_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
