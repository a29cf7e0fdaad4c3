"""Shared by tests/test_command_host.py and tests/test_command_gpu.py: solorl_commands predicted in Python from the oracle's Philox
(oracle.oracle_py.philox) and the table of include/solorl.h -- nothing of the engine's own code -- and the host program
tests/host/command_main.cpp (solorl_amd/csrc/command.hpp compiled alone by g++) with its text protocol.

  decide: draw if restart or draws == 0; else countdown -= 1, draw if countdown == 0
  draw d: key (seed_lo, seed_hi), counter (gid_lo, gid_hi, 2 d, 7): word 0 -> interval = lo + word % (hi - lo + 1); words 1..3 ->
  u = (word >> 8) 2^-24, cmd_k = lo_k + u * (hi_k - lo_k) (Python floats are doubles: the same three operations, each rounded once);
  counter (.., 2 d + 1, 7) word 0: u < zero_prob -> (0, 0, 0); cmd_0^2 + cmd_1^2 < min_lin_norm^2 -> cmd_0 = cmd_1 = 0;
  draws = d + 1, countdown = interval.  Observation word k: float32(cmd_k * obs_scale_k)."""
import numpy as np

from tests.host_util import M32, bits32, hex32, hex64, philox_block, run_host, u24 as uniform  # noqa: F401  (bits32: for the tests)

COMMAND_STREAM = 7


def block(seed, gid, b):
    return philox_block(seed, gid, b, COMMAND_STREAM)


class Params:
    """The members of solorl_command_params but seed, env_id_offset and obs_dim"""

    def __init__(self, lo, hi, interval, zero_prob=0.0, min_lin_norm=0.0, obs_scale=(1.0, 1.0, 1.0)):
        self.lo, self.hi, self.obs_scale = [float(v) for v in lo], [float(v) for v in hi], [float(v) for v in obs_scale]
        self.interval = (int(interval[0]), int(interval[1]))
        self.zero_prob, self.min_lin_norm = float(zero_prob), float(min_lin_norm)


def draw(seed, gid, d, p):
    """draw d of env gid -> (cmd [3] Python floats, interval, zeroed by zero_prob, zeroed by the deadband)"""
    a, b = block(seed, gid, 2 * d), block(seed, gid, 2 * d + 1)
    interval = p.interval[0] + a[0] % (p.interval[1] - p.interval[0] + 1)
    c = []
    for k in range(3):
        width = p.hi[k] - p.lo[k]
        part = uniform(a[1 + k]) * width
        c.append(p.lo[k] + part)
    stand = uniform(b[0]) < p.zero_prob
    if stand:
        c = [0.0, 0.0, 0.0]
    xx, yy, floor2 = c[0] * c[0], c[1] * c[1], p.min_lin_norm * p.min_lin_norm
    dead = xx + yy < floor2
    if dead:
        c[0] = c[1] = 0.0
    return c, interval, stand, dead


class Commands:
    """The memory rows of envs gid0 .. gid0 + n - 1 as solorl_env_command lays them out: call() = one solorl_commands"""

    def __init__(self, seed, gid0, n, p):
        self.seed, self.gid0, self.n, self.p = int(seed), int(gid0), int(n), p
        self.cmd = np.zeros((n, 3), dtype=np.float64)
        self.countdown = np.zeros(n, dtype=np.int32)
        self.draws = np.zeros(n, dtype=np.uint32)

    def call(self, restart=None, mask=None, obs=None):
        """-> (the rows that drew, obs rows [n, D + 3] float32 or None); masked rows of the returned observation are zeros"""
        drew = np.zeros(self.n, dtype=bool)
        for i in range(self.n):
            if mask is not None and not mask[i]:
                continue
            now = (restart is not None and bool(restart[i])) or self.draws[i] == 0
            if not now:
                self.countdown[i] -= 1
                now = self.countdown[i] == 0
            if now:
                d = int(self.draws[i])
                c, interval, _, _ = draw(self.seed, self.gid0 + i, d, self.p)
                self.cmd[i] = c
                self.draws[i] = (d + 1) & M32
                self.countdown[i] = interval
                drew[i] = True
        out = None
        if obs is not None:
            obs = np.asarray(obs, dtype=np.float32)
            out = np.zeros((self.n, obs.shape[1] + 3), dtype=np.float32)
            live = np.ones(self.n, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
            out.view(np.uint32)[live, :obs.shape[1]] = obs.view(np.uint32)[live]
            out[live, obs.shape[1]:] = self.words()[live]
        return drew, out

    def words(self):
        """float32 [n, 3]: the observation words of the commands held now"""
        return np.array([[np.float32(float(self.cmd[i, k]) * self.p.obs_scale[k]) for k in range(3)] for i in range(self.n)], dtype=np.float32).reshape(self.n, 3)

    def rows(self):
        """uint32 [n, 8]: the memory rows' words"""
        w = np.zeros((self.n, 8), dtype=np.uint32)
        w[:, :6] = np.ascontiguousarray(self.cmd).view(np.uint32)
        w[:, 6], w[:, 7] = self.countdown.view(np.uint32), self.draws
        return w


# ---- the host program (tests/host/command_main.cpp: host_util.build_host("command_main"))
def host_commands(exe, seed, gid0, n, D, p, flags, masks, obs):
    """T calls on n zeroed rows in one run.  flags: [T] strings of n characters ('1' restart, '0' none) or '-' (restart == NULL);
    masks: [T] strings of n characters or '-' (mask == NULL); obs: float32 [T, n, D], or None with D == 0 (the no-observation form).
    -> (rows uint32 [T, n, 8], cmd_out float64 bits uint64 [T, n, 3], obs_out uint32 [T, n, D + 3] or None); the words of a masked row are
    what the program's buffers held before the call (rows: the last call's; cmd_out and obs_out: a fill pattern of 0xAA bytes)"""
    T = len(flags)
    head = "%d %d %d %d %d" % (seed, gid0, n, D, T)
    pw = hex64(list(p.lo) + list(p.hi) + list(p.obs_scale) + [p.zero_prob, p.min_lin_norm])
    text = ["%s %s %d %d\n" % (head, pw, p.interval[0], p.interval[1])]
    for t in range(T):
        text.append("%s %s %s\n" % (flags[t], masks[t], hex32(obs[t]) if D else ""))
    lines = run_host(exe, input="".join(text)).splitlines()
    assert len(lines) == T * n
    rows = np.zeros((T, n, 8), dtype=np.uint32)
    cmd = np.zeros((T, n, 3), dtype=np.uint64)
    out = np.zeros((T, n, D + 3), dtype=np.uint32) if D else None
    for k, line in enumerate(lines):
        w = line.split()
        t, i = divmod(k, n)
        rows[t, i] = [int(v, 16) for v in w[:8]]
        cmd[t, i] = [int(v, 16) for v in w[8:11]]
        if D:
            out[t, i] = [int(v, 16) for v in w[11:]]
    return rows, cmd, out
