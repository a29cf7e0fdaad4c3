"""Time-limit bootstrapping of the returns (include/solorl.h solorl_compute_returns_tl): the rollout both test files build, and the
returns it must give, restated as a plain fp64 double loop from the header's formulas -- nothing of the storage's or the kernel's code."""
import numpy as np
import torch

GAMMA, LAM = 0.99, 0.95


def make_case(T, N, seed=0):
    """dict of float32 / uint8 numpy arrays: rewards [T, N], values [T + 1, N], masks [T + 1, N], timeouts [T, N], next_value [N].
    Random everywhere -- episode ends on ~15 % of the steps, flags on half of ALL steps, so most flags stand where m == 1 and must be
    ignored -- and, from T = 9 and N = 5 on, the named cases on envs 0..4:
      0  a timeout at t = 0              1  a timeout at t = T - 1 (the bootstrap stands where next_value would)
      2  timeouts on two steps running   3  an episode end without the flag (a fall)     4  a flag where m == 1
    (T, N) = (1, 1): the one step is a timeout, t = 0 = T - 1."""
    g = np.random.default_rng(seed)
    c = dict(rewards=g.standard_normal((T, N)).astype(np.float32), values=g.standard_normal((T + 1, N)).astype(np.float32),
             masks=(g.random((T + 1, N)) > 0.15).astype(np.float32), timeouts=(g.random((T, N)) > 0.5).astype(np.uint8),
             next_value=g.standard_normal(N).astype(np.float32))
    m, f = c["masks"], c["timeouts"]
    if T >= 9 and N >= 5:
        m[1, 0], f[0, 0] = 0, 1
        m[T, 1], f[T - 1, 1] = 0, 1
        m[4, 2] = m[5, 2] = 0
        f[3, 2] = f[4, 2] = 1
        m[3, 3], f[2, 3] = 0, 0
        m[6, 4], f[5, 4] = 1, 1
    else:
        m[T, 0], f[T - 1, 0] = 0, 1
    return c


def reference_returns(c, use_gae, gamma=GAMMA, lam=LAM, bootstrap=True):
    """-> (returns [T + 1, N], values [T + 1, N] after the call), fp64.  ``bootstrap=False``: the flags are not looked at."""
    r, m, f = (c[k].astype(np.float64) for k in ("rewards", "masks", "timeouts"))
    v = c["values"].astype(np.float64).copy()
    T, N = r.shape
    ret = np.zeros((T + 1, N))
    for n in range(N):
        if use_gae:
            v[T, n] = c["next_value"][n]
            adv = 0.0
            for t in range(T - 1, -1, -1):
                tl = bootstrap and m[t + 1, n] == 0 and f[t, n] != 0
                delta = r[t, n] + gamma * (v[t, n] if tl else v[t + 1, n] * m[t + 1, n]) - v[t, n]
                adv = delta + gamma * lam * m[t + 1, n] * adv
                ret[t, n] = adv + v[t, n]
        else:
            ret[T, n] = c["next_value"][n]
            for t in range(T - 1, -1, -1):
                tl = bootstrap and m[t + 1, n] == 0 and f[t, n] != 0
                ret[t, n] = r[t, n] + gamma * (v[t, n] if tl else ret[t + 1, n] * m[t + 1, n])
    return ret, v


def storage_of(c, device, bootstrap=True, flags=True):
    """a RolloutStorage holding the case (``flags=False``: the timeout rows stay zero)"""
    from solorl_amd.ppo.storage import RolloutStorage
    T, N = c["rewards"].shape
    s = RolloutStorage(T, N, (3,), 2, device, bootstrap_timeouts=bootstrap)
    s.rewards.copy_(torch.from_numpy(c["rewards"]).unsqueeze(-1))
    s.value_preds.copy_(torch.from_numpy(c["values"]).unsqueeze(-1))
    s.masks.copy_(torch.from_numpy(c["masks"]).unsqueeze(-1))
    if bootstrap and flags:
        s.timeouts.copy_(torch.from_numpy(c["timeouts"]).unsqueeze(-1))
    return s


def next_value_of(c, device):
    return torch.from_numpy(c["next_value"]).unsqueeze(-1).to(device)
