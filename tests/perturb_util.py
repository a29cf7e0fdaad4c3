"""Shared by tests/test_perturb_host.py and tests/test_perturb_gpu.py: the kick schedule of solorl_perturb predicted in Python from the
oracle's Philox (oracle.oracle_py.philox) and the draw table of include/solorl.h -- nothing of the engine's own code.

  key (seed_lo, seed_hi), counter (gid_lo, gid_hi, block, 4); block 0 word 0 -> first countdown; kick j: block 1 + 2j words 0..2 -> lin,
  word 3 -> next countdown; block 2 + 2j words 0..2 -> ang; u = (word >> 8) 2^-24, component = (2u - 1) max in double (Python floats are
  doubles: the same two operations), exactly +0.0 for max == 0; countdown = lo + word % (hi - lo + 1)."""
import numpy as np

from tests.host_util import bits64 as bits, philox_block, u24  # noqa: F401  (bits: for the tests)

STREAM = 4


def block(seed, gid, b):
    return philox_block(seed, gid, b, STREAM)


def countdown(word, lo, hi):
    return lo + word % (hi - lo + 1)


def component(word, m):
    if m == 0.0:
        return 0.0
    return (2.0 * u24(word) - 1.0) * m


def first_countdown(seed, gid, lo, hi):
    return countdown(block(seed, gid, 0)[0], lo, hi)


def kick(seed, gid, j, lo, hi, amps):
    """kick j of env gid -> (six doubles: lin x y z, ang x y z; countdown to kick j + 1)"""
    a, b = block(seed, gid, 1 + 2 * j), block(seed, gid, 2 + 2 * j)
    k = [component(a[i], amps[i]) for i in range(3)] + [component(b[i], amps[3 + i]) for i in range(3)]
    return np.array(k, dtype=np.float64), countdown(a[3], lo, hi)


class Schedule:
    """The schedule of envs gid0 .. gid0 + N - 1: call() = one solorl_perturb -> the [N, 6] kicks of that call"""

    def __init__(self, seed, gid0, N, interval, amps):
        self.seed, self.gid0, self.N = int(seed), int(gid0), int(N)
        self.lo, self.hi = interval
        self.amps = [float(a) for a in amps]
        self.countdown = np.array([first_countdown(self.seed, self.gid0 + i, self.lo, self.hi) for i in range(self.N)], dtype=np.int32)
        self.kicks = np.zeros(self.N, dtype=np.int64)

    def call(self):
        out = np.zeros((self.N, 6), dtype=np.float64)
        self.countdown -= 1
        for i in np.nonzero(self.countdown <= 0)[0]:
            out[i], self.countdown[i] = kick(self.seed, self.gid0 + int(i), int(self.kicks[i]), self.lo, self.hi, self.amps)
            self.kicks[i] += 1
        return out
