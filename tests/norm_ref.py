"""fp64 restatement of the reference's VecNormalize arithmetic (agents/running_mean_std.py:18-39 RunningMeanStd.update /
update_mean_var_count_from_moments, :96-121 VecNormalize.step / _obfilt / reset), formula by formula and in its order -- the yardstick
the engine's kernels are held to.  The reference itself keeps the observation statistics in float32 (its obs are float32) and the
return statistics in float64; tests/golden/norm_golden.npz records how far that is from this restatement (tests/test_norm_cpu.py checks
this file against it).  numpy only; shared by the CPU and the GPU tests."""
import numpy as np


def merge_moments(mean, var, count, batch_mean, batch_var, batch_count):
    """running_mean_std.py:28-39"""
    delta = batch_mean - mean
    tot_count = count + batch_count
    new_mean = mean + delta * batch_count / tot_count
    m_a = var * count
    m_b = batch_var * batch_count
    M2 = m_a + m_b + np.square(delta) * count * batch_count / tot_count
    return new_mean, M2 / tot_count, tot_count


class Stats:
    def __init__(self, shape=()):
        self.mean, self.var, self.count = np.zeros(shape, np.float64), np.ones(shape, np.float64), 1e-4      # :13-16

    def update(self, x):                                                                                  # :18-22
        x = np.asarray(x, np.float64)
        self.mean, self.var, self.count = merge_moments(self.mean, self.var, self.count, x.mean(axis=0), x.var(axis=0), x.shape[0])

    def flat(self):
        """the C ABI's `stats` layout: mean[D], var[D], count"""
        return np.concatenate([np.reshape(self.mean, -1), np.reshape(self.var, -1), [self.count]]).astype(np.float64)


class NormRef:
    def __init__(self, n, D, clipob=10.0, cliprew=10.0, gamma=0.99, epsilon=1e-8):
        self.ob, self.rt, self.ret = Stats((D,)), Stats(()), np.zeros(n, np.float64)
        self.clipob, self.cliprew, self.gamma, self.epsilon = clipob, cliprew, gamma, epsilon

    def obs(self, x, update=True):
        """_obfilt (:109-116) for one row [n][D] -> float64 [n][D], not yet rounded to float32"""
        x = np.asarray(x, np.float64)
        if update:
            self.ob.update(x)
        return np.clip((x - self.ob.mean) / np.sqrt(self.ob.var + self.epsilon), -self.clipob, self.clipob)

    def rewards(self, r, done, update=True):
        """the reward half of step (:98-105) for one row [n] -> float64 [n]"""
        r = np.asarray(r, np.float64)
        self.ret = self.ret * self.gamma + r
        if update:
            self.rt.update(self.ret)
        out = np.clip(r / np.sqrt(self.rt.var + self.epsilon), -self.cliprew, self.cliprew)
        self.ret[np.asarray(done).astype(bool)] = 0.0
        return out

    def reset(self):
        self.ret = np.zeros_like(self.ret)                                                                # :119


def ulp32(x):
    """one float32 unit in the last place at |x| (the spacing above |x|; the smallest normal's for tiny values)"""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), np.finfo(np.float32).tiny).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)
