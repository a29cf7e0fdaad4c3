"""Observation noise and actuation (include/solorl.h solorl_obs_noise / solorl_actuate) without a GPU.

The arithmetic of both kernels is solorl_amd/csrc/channel.hpp, plain host-and-device functions: tests/host/channel_main.cpp compiles them
alone with g++ (no -march=native, contraction off) and its rows are compared bitwise with tests/channel_util.py -- the oracle's Philox
and the two tables of the header.  The same stand-alone program runs the boundary shapes under AddressSanitizer and UBSan; it is never
loaded into python.  Then the draws' sign and spread, and the divisors of channel.noise_scales against the oracle's observation."""
import math

import numpy as np
import pytest

from solorl_amd import channel
from solorl_amd.config import default_config, ROBOT_SOLO8, ROBOT_SOLO12, TASK_WALK, TASK_POINTGOAL
from tests import channel_util as cu
from tests.host_util import build_host, san_flags

DIMS = (30, 38, 42, 76, 210)
COUNTS = (0, 1, 2, 2 ** 32 - 1)


@pytest.fixture(scope="module")
def exe():
    return build_host("channel_main")


def pairs():
    """200 (seed, gid): small and large seeds, gids above 2^32"""
    rng = np.random.default_rng(20)
    seeds = [0, 1, 5, 2301, 0xFFFFFFFF, 0x123456789ABCDEF, 2 ** 64 - 1]
    gids = [0, 1, 3, 257, 65535, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 3 * 2 ** 32 + 11, 2 ** 40 + 12345, 2 ** 62 + 1]
    out = [(seeds[k % len(seeds)] if k % 3 else int(rng.integers(0, 2 ** 63)), gids[k % len(gids)] if k % 4 else int(rng.integers(2 ** 32, 2 ** 62)))
           for k in range(200)]
    assert sum(1 for _, g in out if g >= 2 ** 32) >= 60
    return out


def noise_case(rng, D):
    """scales with zeros, inputs with -0.0 and a NaN (one of each under a zero scale and under a non-zero one)"""
    scale = rng.uniform(0.0, 0.2, D).astype(np.float32)
    scale[rng.choice(D, D // 4, replace=False)] = 0.0
    x = rng.uniform(-2.0, 2.0, D).astype(np.float32)
    zero, live = np.nonzero(scale == 0.0)[0], np.nonzero(scale != 0.0)[0]
    x[zero[0]], x[zero[1]] = -0.0, np.nan
    x[live[0]], x[live[1]] = -0.0, np.nan
    return scale, x


def test_host_noise_rows_equal_the_python_prediction(exe):
    rng = np.random.default_rng(5)
    cases = []
    for k, (seed, gid) in enumerate(pairs()):
        D, count = DIMS[k % len(DIMS)], COUNTS[(k // len(DIMS)) % len(COUNTS)]
        scale, x = noise_case(rng, D)
        cases.append((seed, gid, count, scale, x, k % 2))
    assert {(len(c[4]), c[2]) for c in cases} == {(D, c) for D in DIMS for c in COUNTS}      # every D at every count
    got = cu.host_noise(exe, cases)
    changed = 0
    for (seed, gid, count, scale, x, _), (y, after) in zip(cases, got):
        want = cu.noise_row(seed, gid, count, scale, x)
        assert np.array_equal(y, cu.bits32(want)), (seed, gid, count, len(x))
        assert after == (count + 1) % 2 ** 32
        zero = scale == 0.0
        assert np.array_equal(y[zero], cu.bits32(x)[zero])                                   # -0.0 and the NaN's payload survive
        e = cu.noise_e(seed, gid, count, len(x), scale)
        assert np.all(np.abs(e) <= scale.astype(np.float64)) and np.all(e[zero] == 0.0)
        changed += int(np.count_nonzero(y != cu.bits32(x)))
    assert changed > 5000                                                                    # (the comparison was not one of copies)


ACT_CASES = [(A, lo, hi, r) for A in (8, 12) for lo, hi in ((0, 0), (0, 4), (2, 2), (4, 4)) for r in (0.0, 0.2)]
RESTARTS = (0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0)        # 12 calls; call 0 restarts by itself: zeroed memory, restart == NULL
ACT_GIDS = (0, 1, 2, 3, 5, 2 ** 32 + 7, 2 ** 40 + 12345, 2 ** 62 + 1)


def act_actions(A, gid):
    return np.random.default_rng(gid % 9973 + A).uniform(-1.0, 1.0, (len(RESTARTS), A)).astype(np.float32)


def test_the_actuator_cases_reach_every_latency_and_both_signs_of_a_gain():
    lat = {cu.latency(7, g, e, 0, 4) for g in ACT_GIDS for e in range(3)}
    assert lat == {0, 1, 2, 3, 4}, lat
    gains = [float(cu.gain(7, g, e, j, 0.2)) for g in ACT_GIDS for e in range(3) for j in range(12)]
    assert min(gains) < 1.0 < max(gains) and 0.8 <= min(gains) and max(gains) <= 1.2
    assert all(float(cu.gain(7, g, 0, j, 0.0)) == 1.0 for g in ACT_GIDS for j in range(12))


@pytest.mark.parametrize("A,lo,hi,r", ACT_CASES)
def test_host_actuator_rows_equal_the_python_prediction(exe, A, lo, hi, r):
    for gid in ACT_GIDS:
        actions = act_actions(A, gid)
        out, rows = cu.host_actuate(exe, 7, gid, A, lo, hi, r, actions, RESTARTS)
        ref = cu.Actuator(7, gid, 1, A, lo, hi, r)
        for t in range(len(RESTARTS)):
            want = ref.call(actions[t:t + 1], None if t == 0 else [RESTARTS[t]])
            assert np.array_equal(out[t], cu.bits32(want[0])), (gid, t)
            assert np.array_equal(rows[t], ref.rows()[0]), (gid, t)
            start = max(s for s in range(t + 1) if s == 0 or RESTARTS[s])             # the call that began this episode
            assert lo <= ref.latency[0] <= hi and ref.fill[0] == min(t - start + 1, hi)
            if r == 0.0:                                   # nothing is multiplied: the applied action is a buffered raw action, bit for bit
                assert any(np.array_equal(out[t], cu.bits32(actions[s])) for s in range(t + 1))
            assert np.all(rows[t][:48].reshape(4, 12)[hi:] == 0) and np.all(rows[t][:60].reshape(5, 12)[:, A:] == 0)   # never written
        assert ref.episodes[0] == 1 + sum(RESTARTS[1:])


def test_boundary_shapes_under_the_sanitizers(tmp_path):
    """The same stand-alone program with AddressSanitizer and UBSan, on D = 210 and delay_max = 4 (its buffers are heap blocks of exactly
    D and 64 words: an access past either ends the run)"""
    san = build_host("channel_main", san_flags("channel_main"), tmp_path)
    rng = np.random.default_rng(9)
    cases = []
    for k, count in enumerate(COUNTS):
        scale, x = noise_case(rng, 210)
        cases.append((2301, 2 ** 32 + k, count, scale, x, k % 2))
    for (seed, gid, count, scale, x, _), (y, after) in zip(cases, cu.host_noise(san, cases)):
        assert np.array_equal(y, cu.bits32(cu.noise_row(seed, gid, count, scale, x)))
    for A in (8, 12):
        for lo in (0, 4):
            actions = act_actions(A, 3)
            out, rows = cu.host_actuate(san, 7, 3, A, lo, 4, 0.2, actions, RESTARTS)
            ref = cu.Actuator(7, 3, 1, A, lo, 4, 0.2)
            for t in range(len(RESTARTS)):
                want = ref.call(actions[t:t + 1], None if t == 0 else [RESTARTS[t]])
                assert np.array_equal(out[t], cu.bits32(want[0])) and np.array_equal(rows[t], ref.rows()[0])


def test_sign_and_spread_of_the_noise(exe):
    """M = 2^20 draws of one component with half-width s: u = k 2^-24 with k uniform in 0 .. 2^24 - 1, so e = (2u - 1) s has mean
    -s 2^-24 and variance (s^2 / 3)(1 - 2^-48).  The sample mean of M draws has standard deviation s / sqrt(3 M): five of them bound it
    (the offset of the mean is 1e-4 of that).  The sample variance has relative standard deviation sqrt(4/5 / M) = 8.7e-4 (the fourth
    moment of a uniform draw is s^4 / 5): 1 % is 11 of them."""
    M, s, D, c = 2 ** 20, 0.5, 42, 5
    line = cu.run_host(exe, "S 2301 %d 0 %d %d %d %08x\n" % (2 ** 32 + 9, M, D, c, int(cu.bits32([s])[0])))[0]
    e = np.array([int(v, 16) for v in line.split()], dtype=np.uint32).view(np.float32).astype(np.float64)
    assert e.shape == (M,)
    assert np.array_equal(e[:8], [cu.noise_e(2301, 2 ** 32 + 9, k, D, [0.0] * c + [s] + [0.0] * (D - c - 1))[c] for k in range(8)])   # (exact: s is a power of two)
    assert abs(e.mean()) < 5 * s / math.sqrt(3 * M), e.mean()
    assert abs(e.var() / (s * s / 3) - 1.0) < 0.01, e.var()
    assert e.min() < -0.99 * s and e.max() > 0.99 * s and np.all(np.abs(e) <= s)


def quat_about(axis, angle):
    q = [0.0, 0.0, 0.0, math.cos(angle / 2)]
    q[axis] = math.sin(angle / 2)
    return q


@pytest.mark.parametrize("robot", [ROBOT_SOLO8, ROBOT_SOLO12])
@pytest.mark.parametrize("task", [TASK_WALK, TASK_POINTGOAL])
@pytest.mark.parametrize("history", [0, 1])
def test_noise_scales_divide_by_the_observation_scaling_of_the_oracle(robot, task, history):
    """Each group's state member is moved by delta through the oracle's get_state / set_state and the observation must move by
    delta / divisor -- the divisor noise_scales uses -- in the level-0 block and in the history difference block alike."""
    from oracle import oracle_py
    from oracle.oracle_py import Oracle
    cfg = default_config(robot, task)
    cfg.num_history_stack = history
    n, D = cfg.n_joints, cfg.state_dim
    orc = Oracle(cfg, 1, seed=3)
    orc.reset()
    base = orc.get_state(0)
    base.quat[:] = quat_about(0, 0.3)
    assert abs(oracle_py.euler_from_quat(list(base.quat))[0] - 0.3) < 1e-12
    orc.set_state(0, base)
    obs0 = orc.get_observation()[0]
    delta = 0.1
    half = {"height": 0.02, "orientation": 0.05, "lin_vel": 0.1, "ang_vel": 0.2, "joint_pos": 0.03, "joint_vel": 1.5}
    if task == TASK_POINTGOAL:
        half["position"] = 0.04
    scales = channel.noise_scales(cfg, half, history=0.5).numpy().astype(np.float64)
    assert scales.shape == (cfg.obs_dim,)
    seen = np.zeros(D, dtype=bool)
    for name, first, count, div in channel.group_layout(cfg):
        for k in range(count):
            c = first + k
            seen[c] = True
            if name is None:
                assert scales[c] == 0.0 and (history == 0 or scales[D + c] == 0.0)
                continue
            s = orc.get_state(0)
            if name == "height":
                s.pos[2] += delta
            elif name == "orientation":
                ang = [0.3, 0.0, 0.0]
                ang[k] += delta
                # one axis at a time: roll 0.3 -> 0.4, or roll 0 and pitch / yaw 0 -> 0.1 against a base of its own
                s.quat[:] = quat_about(k, 0.3 + delta) if k == 0 else quat_about(k, delta)
            elif name == "lin_vel":
                s.lin_vel[k] += delta
            elif name == "ang_vel":
                s.ang_vel[k] += delta
            elif name == "joint_pos":
                s.q[k] += delta
            elif name == "joint_vel":
                s.qd[k] += delta
            elif name == "position":
                s.pos[k] += delta
            orc.set_state(0, s)
            obs = orc.get_observation()[0]
            ref = obs0
            if name == "orientation" and k > 0:          # the base of pitch and yaw: no rotation at all
                s0 = orc.get_state(0)
                s0.quat[:] = [0.0, 0.0, 0.0, 1.0]
                orc.set_state(0, s0)
                ref = orc.get_observation()[0]
            assert abs((obs[c] - ref[c]) - delta / div) < 1e-9, (name, k, obs[c] - ref[c], delta / div)
            assert abs(scales[c] - np.float32(half[name] / div)) < 1e-9, (name, k)
            if history:
                assert abs((obs[D + c] - ref[D + c]) - delta / div) < 1e-9, (name, k)
                assert abs(scales[D + c] - np.float32(0.5 * half[name] / div)) < 1e-9, (name, k)
            orc.set_state(0, base)
    assert seen.all()
    divisors = {name: div for name, _, _, div in channel.group_layout(cfg) if name}
    assert divisors == dict(height=1.0, orientation=2.0, lin_vel=1.0, ang_vel=1.0, joint_pos=cfg.joint_limit, joint_vel=100.0,
                            **({"position": 2.0} if task == TASK_POINTGOAL else {}))


def test_noise_scales_refuses_unknown_groups_by_name():
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    with pytest.raises(ValueError, match="hieght"):
        channel.noise_scales(cfg, {"hieght": 0.1})
    with pytest.raises(ValueError, match="position"):
        channel.noise_scales(cfg, {"position": 0.1})
    with pytest.raises(ValueError, match="groups"):
        channel.scales_from_dict(cfg, {"height": 0.1})
    assert float(channel.noise_scales(cfg, {}).abs().sum()) == 0.0
