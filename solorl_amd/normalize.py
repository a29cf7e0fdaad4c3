"""Running observation / return normalisation -- the reference's ``VecNormalize`` with its ``RunningMeanStd``
(agents/running_mean_std.py:11-39, :73-127) -- on the device: the statistics live in fp64 device tensors and every update and
scaling is ``solorl_normalize_obs`` / ``solorl_normalize_rewards`` (include/solorl.h, csrc/solorl_norm.hip) on the caller's
current stream.  torch owns the buffers only.

  RunningMeanStd   the host-side value (numpy ``mean``, ``var``, ``count`` as the reference's: what a checkpoint carries)
  VecNormalizer    the device state of one vec-env: statistics, the per-env discounted-return accumulators, scratch
"""
import ctypes as C

import numpy as np
import torch

from . import _native


class RunningMeanStd:
    """agents/running_mean_std.py:11-16: mean 0, var 1, count epsilon.  fp64 (the device keeps the statistics in fp64)."""

    def __init__(self, epsilon=1e-4, shape=()):
        self.mean = np.zeros(shape, np.float64)
        self.var = np.ones(shape, np.float64)
        self.count = float(epsilon)

    def to_device(self, device, out=None):
        """-> float64 tensor [2 D + 1] = mean[D], var[D], count (D = 1 for a scalar statistic): the C ABI's ``stats``"""
        flat = np.concatenate([np.asarray(self.mean, np.float64).reshape(-1), np.asarray(self.var, np.float64).reshape(-1),
                               np.asarray([self.count], np.float64)])
        t = torch.from_numpy(flat)
        if out is None:
            return t.to(device)
        if tuple(out.shape) != tuple(t.shape):
            raise ValueError("statistics of %d columns do not fit a device tensor of %d values" % ((t.numel() - 1) // 2, out.numel()))
        out.copy_(t)
        return out

    def from_device(self, stats):
        """Fills this object from a ``stats`` tensor (one device -> host copy); keeps the shape of ``mean``."""
        h = stats.detach().cpu().numpy().astype(np.float64)
        D = (h.size - 1) // 2
        shape = np.shape(self.mean) if np.size(self.mean) == D else (D,)
        self.mean, self.var, self.count = h[:D].reshape(shape).copy(), h[D:2 * D].reshape(shape).copy(), float(h[2 * D])
        return self

    def update(self, x):
        """agents/running_mean_std.py:18-39 on the host, fp64 (not used by the engine: for callers that kept using it)"""
        x = np.asarray(x, np.float64)
        bm, bv, bn = x.mean(axis=0), x.var(axis=0), x.shape[0]
        delta, tot = bm - self.mean, self.count + bn
        self.mean = self.mean + delta * bn / tot
        self.var = (self.var * self.count + bv * bn + np.square(delta) * self.count * bn / tot) / tot
        self.count = tot


class VecNormalizer:
    """Device state and launches of VecNormalize for ``n`` envs with ``obs_dim`` observations."""

    def __init__(self, n, obs_dim, device, norm_obs, norm_ret, clipob=10.0, cliprew=10.0, gamma=0.99, epsilon=1e-8):
        self.n, self.D, self.device = int(n), int(obs_dim), device
        self.clipob, self.cliprew, self.gamma, self.epsilon = float(clipob), float(cliprew), float(gamma), float(epsilon)
        self.L = _native.lib()
        self.ob_stats = RunningMeanStd(shape=(self.D,)).to_device(device) if norm_obs else None
        self.ret_stats = RunningMeanStd(shape=()).to_device(device) if norm_ret else None
        self.ret = torch.zeros(self.n, dtype=torch.float64, device=device)           # running_mean_std.py:90
        self._scratch = {}
        for D in ([self.D] if norm_obs else []) + ([1] if norm_ret else []):        # one-row calls: allocated here, not inside a capture
            self.scratch(1, D)

    def scratch(self, rows, D):
        s = self._scratch.get((rows, D))
        if s is None:
            k = self.L.solorl_norm_scratch_count(rows, self.n, D)
            if k < 1:
                raise _native.SoloRLError("running normalisation: %d rows x %d envs x %d columns is out of range" % (rows, self.n, D))
            s = self._scratch[(rows, D)] = torch.empty(k, dtype=torch.float64, device=self.device)
        return s

    def obs(self, x, rows, update, out=None):
        """x: contiguous float32 [rows, n, D] (or [n, D] with rows = 1) on the device, normalised in place (or into ``out``)"""
        out = x if out is None else out
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_normalize_obs(C.c_void_p(self.ob_stats.data_ptr()), rows, self.n, self.D, C.c_void_p(x.data_ptr()),
                                                      C.c_void_p(out.data_ptr()), 1 if update else 0, self.clipob, self.epsilon,
                                                      C.c_void_p(self.scratch(rows, self.D).data_ptr()), self.device.index or 0, _native.stream(self.device)))
        return out

    def rewards(self, r, done, rows, update):
        """r: contiguous float32 [rows, n] (any trailing 1), done: uint8 [rows, n]; rewards rewritten in place.  Without return
        normalisation nothing is launched (the accumulators are only read by it)."""
        if self.ret_stats is None:
            return r
        with torch.cuda.device(self.device):
            _native.check(self.L.solorl_normalize_rewards(C.c_void_p(self.ret_stats.data_ptr()), C.c_void_p(self.ret.data_ptr()), rows, self.n,
                                                          C.c_void_p(r.data_ptr()), C.c_void_p(done.data_ptr()), 1 if update else 0, self.gamma,
                                                          self.cliprew, self.epsilon, C.c_void_p(self.scratch(rows, 1).data_ptr()),
                                                          self.device.index or 0, _native.stream(self.device)))
        return r
