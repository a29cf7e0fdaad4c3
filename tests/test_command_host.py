"""Velocity commands (include/solorl.h solorl_commands) without a GPU.

The arithmetic of the kernel is solorl_amd/csrc/command.hpp, plain host-and-device functions: tests/host/command_main.cpp compiles them
alone with g++ (no -march=native, contraction off) and its rows are compared bitwise with tests/command_util.py -- the oracle's Philox
and the table of the header.  The same stand-alone program runs the boundary shapes under AddressSanitizer and UBSan; it is never loaded
into python.  One test needs the prediction only: the seeds and ranges used here and on the GPU reach every branch of the table."""
import numpy as np
import pytest

from tests import command_util as cu
from tests.host_util import build_host, san_flags

SEED = 2301
INTERVAL = (2, 5)
# the ranges of the host and the GPU tests: a walk task's (both signs, a zero command now and then, a deadband), and a joystick's
WALK = cu.Params(lo=(-1.0, -0.5, -1.0), hi=(1.0, 0.5, 1.0), interval=INTERVAL, zero_prob=0.15, min_lin_norm=0.3, obs_scale=(2.0, 2.0, 0.25))
FIXED = cu.Params(lo=(0.3, -0.1, 0.7), hi=(0.3, -0.1, 0.7), interval=INTERVAL)
RANGES = {"walk": WALK, "fixed": FIXED}
GID0 = 2 ** 32 - 3                  # the batch straddles the 32-bit boundary of the global env id
CALLS = 40
RESTART_AT = {7: (0, 3), 8: (3,), 20: (1, 2, 5), 33: (4,)}       # call -> the envs restarted by it
MASK_AT = {5: (0, 1, 2, 4), 6: (0, 1, 2, 4), 21: (5,)}           # call -> the live envs (every other call: all)


def schedule(n, calls=CALLS):
    """(flags, masks) of the run: call 0 and every call without an entry pass NULL"""
    flags = ["".join("1" if i in RESTART_AT[t] else "0" for i in range(n)) if t in RESTART_AT else "-" for t in range(calls)]
    masks = ["".join("1" if i in MASK_AT[t] else "0" for i in range(n)) if t in MASK_AT else "-" for t in range(calls)]
    return flags, masks


def bools(s, n):
    return None if s == "-" else [c == "1" for c in s]


def obs_rows(calls, n, D, seed=3):
    """float32 [calls, n, D] with a -0.0 and a NaN that carries a payload in every row"""
    x = np.random.default_rng(seed + D).uniform(-2.0, 2.0, (calls, n, D)).astype(np.float32)
    x[:, :, 0] = -0.0
    x.view(np.uint32)[:, :, D - 1] = 0x7FC12345
    return x


@pytest.fixture(scope="module")
def exe():
    return build_host("command_main")


def check_run(exe, name, n, D, calls=CALLS):
    p = RANGES[name]
    flags, masks = schedule(n, calls)
    obs = obs_rows(calls, n, D) if D else None
    rows, cmd, out = cu.host_commands(exe, SEED, GID0, n, D, p, flags, masks, obs)
    ref = cu.Commands(SEED, GID0, n, p)
    fill32, fill64 = 0xAAAAAAAA, 0xAAAAAAAAAAAAAAAA
    for t in range(calls):
        m = bools(masks[t], n)
        _, want = ref.call(bools(flags[t], n), m, None if obs is None else obs[t])
        live = np.ones(n, dtype=bool) if m is None else np.array(m)
        assert np.array_equal(rows[t], ref.rows()), (name, t)                              # masked rows: the last call's words
        assert np.array_equal(cmd[t][live], np.ascontiguousarray(ref.cmd).view(np.uint64)[live]), (name, t)
        assert np.all(cmd[t][~live] == fill64), (name, t)
        if D:
            assert np.array_equal(out[t][live], want.view(np.uint32)[live]), (name, t)
            assert np.all(out[t][~live] == fill32), (name, t)
            assert np.array_equal(out[t][live][:, :D], obs[t].view(np.uint32)[live])          # -0.0 and the NaN's payload survive
    return ref


@pytest.mark.parametrize("name", sorted(RANGES))
def test_host_rows_equal_the_python_prediction(exe, name):
    ref = check_run(exe, name, 6, 42)
    assert int(ref.draws.min()) >= 8                        # 40 calls at 2..5 steps between draws
    check_run(exe, name, 6, 0)                              # the no-observation form
    if name == "fixed":
        assert np.all(ref.cmd == np.array(FIXED.lo))        # lo == hi: exactly lo


def test_boundary_shapes_under_the_sanitizers(tmp_path):
    """The same stand-alone program with AddressSanitizer and UBSan on n = 1 and D in {1, 42, 210} (its observation buffers are heap
    blocks of exactly D and D + 3 floats: an access past either ends the run)"""
    san = build_host("command_main", san_flags("command_main"), tmp_path)
    for D in (1, 42, 210):
        p = WALK
        obs = obs_rows(12, 1, D)
        flags = ["-"] + ["1" if t in (4, 9) else "0" for t in range(1, 12)]
        rows, cmd, out = cu.host_commands(san, SEED, 2 ** 40 + 7, 1, D, p, flags, ["-"] * 12, obs)
        ref = cu.Commands(SEED, 2 ** 40 + 7, 1, p)
        for t in range(12):
            _, want = ref.call(bools(flags[t], 1), None, obs[t])
            assert np.array_equal(rows[t], ref.rows()) and np.array_equal(out[t], want.view(np.uint32)), (D, t)
            assert np.array_equal(cmd[t], np.ascontiguousarray(ref.cmd).view(np.uint64))


def test_the_cases_reach_every_branch_of_the_table():
    """From the prediction alone: over the draws the runs above make (envs GID0 .. GID0 + 5, draws 0 .. 7, which every env reaches) the
    walk ranges give every interval value, a draw zeroed by zero_prob, one zeroed by the deadband, one that passes it, and both signs
    of every component; the fixed ranges give lo whatever the draw."""
    seen = [cu.draw(SEED, GID0 + i, d, WALK) for i in range(6) for d in range(8)]
    assert {s[1] for s in seen} == set(range(INTERVAL[0], INTERVAL[1] + 1))
    assert any(s[2] for s in seen) and any(s[3] and not s[2] for s in seen)
    passed = [s[0] for s in seen if not s[2] and not s[3]]
    assert passed and all(c[0] * c[0] + c[1] * c[1] >= 0.09 - 1e-12 for c in passed)
    for s in seen:
        if s[2]:
            assert s[0] == [0.0, 0.0, 0.0]
        elif s[3]:
            assert s[0][0] == 0.0 and s[0][1] == 0.0 and s[0][2] != 0.0          # the deadband leaves the yaw rate
    for k in range(3):
        vals = [c[k] for c in passed]
        assert min(vals) < 0.0 < max(vals) and WALK.lo[k] <= min(vals) and max(vals) <= WALK.hi[k], k
    for i in range(6):
        for d in range(8):
            c, interval, stand, dead = cu.draw(SEED, GID0 + i, d, FIXED)
            assert c == list(FIXED.lo) and not stand and not dead and INTERVAL[0] <= interval <= INTERVAL[1]
    # the observation words: the product in double, one rounding to float
    ref = cu.Commands(SEED, GID0, 6, WALK)
    ref.call()
    assert np.array_equal(ref.words(), (ref.cmd * np.array(WALK.obs_scale)).astype(np.float32))
