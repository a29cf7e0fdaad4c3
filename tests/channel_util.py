"""Shared by tests/test_channel_host.py and tests/test_channel_gpu.py: solorl_obs_noise and solorl_actuate
predicted in Python from the oracle's Philox (oracle.oracle_py.philox) and the two tables of include/solorl.h -- nothing of the engine's
own code -- and the host program tests/host/channel_main.cpp (solorl_amd/csrc/channel.hpp compiled alone by g++) with its text protocol.

  noise: key (seed_lo, seed_hi), counter (gid_lo, gid_hi, count * B + b mod 2^32, 5), B = ceil(D / 4), word w of block b -> component
  4 b + w; u = (word >> 8) 2^-24, e = (2u - 1) * double(scale) (Python floats are doubles: the same operations, each rounded once),
  out = float32(double(x) + e); scale == 0 keeps x's bits.
  actuation: counter (gid_lo, gid_hi, 4 e, 6) word 0 -> latency = lo + word % (hi - lo + 1); (.., 4 e + 1 + j // 4, 6) word j % 4 ->
  gain = float32(1.0 + (2u - 1) * r); delayed = in if latency == 0 or fill == 0 else buf[min(latency, fill) - 1]; out = delayed (bits)
  if r == 0 else float32(double(gain) * double(delayed)); then the levels move up, buf[0] = in, fill = min(fill + 1, hi)."""
import numpy as np

from tests import host_util
from tests.host_util import M32, bits32, hex32 as _hex, hex64, philox_block as block, u24

NOISE_STREAM, ACTUATE_STREAM = 5, 6
DELAY_MAX = 4


def symmetric(word):
    return 2.0 * u24(word) - 1.0


def noise_e(seed, gid, count, D, scale):
    """the [D] float64 noise of call `count` (0-based) of env gid; exactly 0.0 where scale is 0"""
    B = (D + 3) // 4
    e = np.zeros(D, dtype=np.float64)
    for b in range(B):
        w = block(seed, gid, (count * B + b) & M32, NOISE_STREAM)
        for k in range(4):
            c = 4 * b + k
            if c < D and scale[c] != 0.0:
                e[c] = symmetric(w[k]) * float(np.float32(scale[c]))
    return e


def noise_row(seed, gid, count, scale, x):
    """float32 [D] row x -> the noisy row, bits of x kept where scale is 0"""
    x = np.asarray(x, dtype=np.float32)
    e = noise_e(seed, gid, count, x.shape[0], scale)
    y = (x.astype(np.float64) + e).astype(np.float32)
    keep = np.asarray(scale, dtype=np.float32) == 0.0
    y.view(np.uint32)[keep] = x.view(np.uint32)[keep]
    return y


def noise_rows(seed, gid0, counts, scale, x, mask=None):
    """[n, D] rows of envs gid0 .. -> (noisy rows, counts afterwards); masked rows (mask byte 0) and their counts stay"""
    x = np.asarray(x, dtype=np.float32)
    out, cnt = x.copy(), np.asarray(counts, dtype=np.uint32).copy()
    for i in range(x.shape[0]):
        if mask is None or mask[i]:
            out[i] = noise_row(seed, gid0 + i, int(cnt[i]), scale, x[i])
            cnt[i] = (int(cnt[i]) + 1) & M32
    return out, cnt


def latency(seed, gid, e, lo, hi):
    return lo + block(seed, gid, (4 * e) & M32, ACTUATE_STREAM)[0] % (hi - lo + 1)


def gain(seed, gid, e, j, r):
    w = block(seed, gid, (4 * e + 1 + j // 4) & M32, ACTUATE_STREAM)[j % 4]
    d = symmetric(w) * float(r)
    return np.float32(1.0 + d)


class Actuator:
    """The memory rows of envs gid0 .. gid0 + n - 1 as solorl_env_actuator lays them out: call() = one solorl_actuate"""

    def __init__(self, seed, gid0, n, A, lo, hi, r):
        self.seed, self.gid0, self.n, self.A, self.lo, self.hi, self.r = int(seed), int(gid0), int(n), int(A), int(lo), int(hi), float(r)
        self.buf = np.zeros((n, DELAY_MAX, 12), dtype=np.float32)
        self.gain = np.zeros((n, 12), dtype=np.float32)
        self.latency = np.zeros(n, dtype=np.int32)
        self.fill = np.zeros(n, dtype=np.int32)
        self.episodes = np.zeros(n, dtype=np.uint32)

    def call(self, actions, restart=None):
        a = np.asarray(actions, dtype=np.float32)
        out = np.empty_like(a)
        A = self.A
        for i in range(self.n):
            if (restart is not None and restart[i]) or self.episodes[i] == 0:
                e = int(self.episodes[i])
                self.latency[i] = latency(self.seed, self.gid0 + i, e, self.lo, self.hi)
                for j in range(A):
                    self.gain[i, j] = gain(self.seed, self.gid0 + i, e, j, self.r)
                self.fill[i] = 0
                self.episodes[i] = (e + 1) & M32
            L, F = int(self.latency[i]), int(self.fill[i])
            d = a[i].copy() if (L == 0 or F == 0) else self.buf[i, min(L, F) - 1, :A].copy()
            if self.r == 0.0:
                out[i] = d
            else:
                out[i] = (self.gain[i, :A].astype(np.float64) * d.astype(np.float64)).astype(np.float32)
            for k in range(self.hi - 1, 0, -1):
                self.buf[i, k, :A] = self.buf[i, k - 1, :A]
            if self.hi > 0:
                self.buf[i, 0, :A] = a[i]
            self.fill[i] = min(F + 1, self.hi)
        return out

    def rows(self):
        """uint32 [n, 64]: the memory rows' words"""
        w = np.zeros((self.n, 64), dtype=np.uint32)
        w[:, :48] = self.buf.reshape(self.n, 48).view(np.uint32)
        w[:, 48:60] = self.gain.view(np.uint32)
        w[:, 60], w[:, 61], w[:, 62] = self.latency.view(np.uint32), self.fill.view(np.uint32), self.episodes
        return w


# ---- the host program (tests/host/channel_main.cpp: host_util.build_host("channel_main"))
def run_host(exe, text):
    return host_util.run_host(exe, input=text).splitlines()


def host_noise(exe, cases):
    """cases: [(seed, gid, count, scale float32 [D], x float32 [D], in_place)] -> [(noisy row as uint32 [D], count afterwards)]"""
    text = "".join("N %d %d %d %d %d %s %s\n" % (s, g, c, len(x), int(ip), _hex(sc), _hex(x)) for s, g, c, sc, x, ip in cases)
    out = []
    for line in run_host(exe, text):
        w = line.split()
        out.append((np.array([int(v, 16) for v in w[1:]], dtype=np.uint32), int(w[0])))
    assert len(out) == len(cases)
    return out


def host_actuate_many(exe, seed, gids, A, lo, hi, r, actions, flags):
    """Every env's sequence of calls over zeroed memory, in one run: actions float32 [n, T, A], flags [n] strings of T characters ('1'
    restart, '0' none, '-' restart == NULL) -> (out uint32 [n, T, A], rows uint32 [n, T, 64] after each call)"""
    n, T = len(gids), len(flags[0])
    text = "".join("A %d %d %d %d %d %s %d %s %s\n" % (seed, gids[i], A, lo, hi, hex64(r), T, flags[i], _hex(actions[i])) for i in range(n))
    lines = run_host(exe, text)
    assert len(lines) == n * T
    words = np.array([[int(v, 16) for v in l.split()] for l in lines], dtype=np.uint32).reshape(n, T, A + 64)
    return words[:, :, :A], words[:, :, A:]


def host_actuate(exe, seed, gid, A, lo, hi, r, actions, restarts, null_restart_at=(0,)):
    """One env: actions float32 [T, A], restarts [T] of 0 / 1 -> (out uint32 [T, A], rows uint32 [T, 64]).  The calls listed in
    null_restart_at pass restart == NULL (their restarts entry must be 0)."""
    flags = "".join("-" if t in null_restart_at else str(int(restarts[t])) for t in range(len(actions)))
    out, rows = host_actuate_many(exe, seed, [gid], A, lo, hi, r, [actions], [flags])
    return out[0], rows[0]
