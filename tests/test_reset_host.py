"""solorl_randomize_reset's row arithmetic (solorl_amd/csrc/reset_random.hpp) compiled alone by g++ (tests/host/reset_random_main.cpp)
against the draw table of include/solorl.h restated in numpy (tests/reset_util.py): no GPU.

q, qd, lin_vel, ang_vel, count and the contact words are bitwise; quat and pos.z (sin, cos and the kinematics) to 1e-12; the placing is
checked against the oracle's support points on the OUTPUT rows to 1e-9 m."""
import math

import numpy as np
import pytest

from tests import reset_util as ru
from tests.host_util import build_host, san_flags
from tests.reset_util import W


@pytest.fixture(scope="module")
def exe():
    return build_host("reset_random_main")


def run(exe, robot12, p, rows, count=None, mask=None, live=None, what=""):
    count = np.zeros(rows.shape[0], np.uint32) if count is None else count
    got = ru.host_reset(exe, robot12, p, rows, count, mask)
    want = ru.reference(robot12, p, rows, count, mask, live)
    err = ru.check(got[0], got[1], want[0], want[1], rows, mask, live, what)
    return got, err


@pytest.mark.parametrize("robot12", [0, 1])
def test_full_table(exe, robot12):
    """every half-width set, crafted and random rows, episodes 0 and 3"""
    rows = ru.batch(robot12, 40)
    for k in (0, 3):
        (out, cnt), err = run(exe, robot12, ru.full(robot12), rows, np.full(40, k, np.uint32), what="k=%d" % k)
        print("robot12=%d k=%d: max |quat, pos.z error| %.3e" % (robot12, k, err))
        assert (cnt == k + 1).all()
    nq = 12 if robot12 else 8
    q = out[:, W("q"):W("q") + nq]
    assert (np.abs(q) <= 1.0).all() and (np.abs(q) == 1.0).any(), "the clamp at +-joint_limit is met"
    assert np.allclose(np.linalg.norm(out[:, ru.QUAT], axis=1), 1.0, rtol=0, atol=1e-14) and (out[:, W("quat") + 3] >= 0).all()


@pytest.mark.parametrize("robot12", [0, 1])
@pytest.mark.parametrize("key", ["joint_pos", "joint_vel", "lin_vel", "ang_vel", "yaw", "roll", "pitch", "place_on_ground"])
def test_one_width(exe, robot12, key):
    """every width zero except one: only that member's words change, and the contact cache goes exactly when the pose can change"""
    value = {"joint_pos": 0.3, "joint_vel": 2.0, "lin_vel": 0.5, "ang_vel": 0.7, "yaw": 3.0, "roll": 0.2, "pitch": 0.25, "place_on_ground": 1}[key]
    p = ru.Params(seed=99, id0=3, **{key: value})
    rows = ru.batch(robot12, 16)
    (out, _), _ = run(exe, robot12, p, rows, what=key)
    changed = (ru.bits(out) != ru.bits(rows)).any(axis=0)
    nq = 12 if robot12 else 8
    span = {"joint_pos": (W("q"), nq), "joint_vel": (W("qd"), nq), "lin_vel": (W("lin_vel"), 3), "ang_vel": (W("ang_vel"), 3), "yaw": (W("quat"), 4),
            "roll": (W("quat"), 4), "pitch": (W("quat"), 4), "place_on_ground": (ru.POS_Z, 1)}[key]
    allowed = np.zeros(ru.ROW_WORDS, bool)
    allowed[span[0]:span[0] + span[1]] = True
    pose = key in ("joint_pos", "yaw", "roll", "pitch", "place_on_ground")
    if pose:
        allowed[W("lambda_prev"):W("lambda_prev") + 24] = True
        allowed[ru.MASK_WORD] = True
        assert (out[:, W("lambda_prev"):W("lambda_prev") + 24] == 0).all()
        assert ((out.view(np.uint32)[:, 2 * ru.MASK_WORD] & 0xFFFFFF) == 0).all()
        assert np.array_equal(out.view(np.uint32)[:, 2 * ru.MASK_WORD] >> 24, rows.view(np.uint32)[:, 2 * ru.MASK_WORD] >> 24), "bits 24.. stay"
        assert np.array_equal(out.view(np.uint32)[:, 2 * ru.MASK_WORD + 1], rows.view(np.uint32)[:, 2 * ru.MASK_WORD + 1]), "rng_counter stays"
    assert not changed[~allowed].any(), np.nonzero(changed & ~allowed)[0]
    assert changed[span[0]:span[0] + span[1]].all()


def test_zero_width_keeps_negative_zero(exe):
    rows, names = ru.crafted_rows(1)
    i = names.index("negative zeros")
    p = ru.full(1, joint_pos=[0.0, 0.2] + [0.2] * 10, joint_vel=[1.0, 0.0] + [1.0] * 10, lin_vel=[0.0, 0.3, 0.0], ang_vel=[0.4, 0.0, 0.4],
                yaw=0.0, roll=0.0, pitch=0.0, place_on_ground=0)
    (out, _), _ = run(exe, 1, p, rows)
    for w in (W("q"), W("qd") + 1, W("lin_vel"), W("lin_vel") + 2, W("ang_vel") + 1, W("quat"), ru.POS_Z):
        assert ru.bits(out[i])[w] == 0x8000000000000000, w
    # all widths zero: nothing of any row changes but count
    (out, cnt), _ = run(exe, 1, ru.Params(seed=5), rows)
    assert np.array_equal(ru.bits(out), ru.bits(rows)) and (cnt == 1).all()


def test_solo8_leaves_joints_8_to_11_and_primitives_20_to_23(exe):
    """widths named for joints 8..11 draw nothing on a Solo8, and its lowest point never comes from a shoulder primitive it lacks:
    KinRow writes zeros for those, which would win the minimum over a robot standing above the ground"""
    p = ru.full(0, joint_pos=[0.2] * 12, joint_vel=[1.0] * 12, clearance=0.02)
    rows = ru.batch(0, 24)
    rows[:, ru.POS_Z] = np.abs(rows[:, ru.POS_Z]) + 1.0                 # every point above z = 0 before the call
    (out, _), _ = run(exe, 0, p, rows)
    assert np.array_equal(ru.bits(out[:, W("q") + 8:W("q") + 12]), ru.bits(rows[:, W("q") + 8:W("q") + 12]))
    assert np.array_equal(ru.bits(out[:, W("qd") + 8:W("qd") + 12]), ru.bits(rows[:, W("qd") + 8:W("qd") + 12]))
    for r in out:
        assert abs(ru.support_z(0, r).min() - 0.02) <= ru.TOL_PLACE
    only = ru.Params(seed=3, joint_pos=[0.0] * 8 + [0.2] * 4)           # nothing a Solo8 has: no draw, and the contact cache stays
    (out, _), _ = run(exe, 0, only, rows)
    assert np.array_equal(ru.bits(out), ru.bits(rows))


@pytest.mark.parametrize("robot12", [0, 1])
def test_masked_rows_against_poison(exe, robot12):
    rows = ru.batch(robot12, 20)
    mask = (np.arange(20) % 3 != 1).astype(np.uint8)
    mask[5] = 255
    count = np.arange(20, dtype=np.uint32) * 7
    (out, cnt), _ = run(exe, robot12, ru.full(robot12), rows, count, mask)
    assert np.array_equal(cnt[mask == 0], count[mask == 0]) and np.array_equal(cnt[mask != 0], count[mask != 0] + 1)


def test_episodes_differ_and_wrap(exe):
    rows = np.repeat(ru.batch(1, 1), 4, axis=0)
    p = ru.full(1, id0=0)
    outs = [ru.host_reset(exe, 1, p, rows, np.full(4, k, np.uint32))[0] for k in (0, 1, 2)]
    for a in range(3):
        for b in range(a + 1, 3):
            assert (ru.bits(outs[a][0])[:ru.HEAD_WORDS] != ru.bits(outs[b][0])[:ru.HEAD_WORDS]).sum() > 30, "k = %d and %d draw differently" % (a, b)
    assert (ru.bits(outs[0][0])[:ru.HEAD_WORDS] != ru.bits(outs[0][1])[:ru.HEAD_WORDS]).sum() > 30, "two envs draw differently"
    run(exe, 1, p, rows, np.array([0, 1, (1 << 28) - 1, 0xFFFFFFFF], np.uint32), what="large k")      # (count wraps as a uint32)


@pytest.mark.parametrize("robot12", [0, 1])
def test_two_shards_draw_like_one_batch(exe, robot12):
    n = 12
    rows = ru.batch(robot12, 2 * n)
    p = ru.full(robot12, id0=1 << 33)
    count = np.arange(2 * n, dtype=np.uint32)
    whole, wc = ru.host_reset(exe, robot12, p, rows, count)
    for s in (0, 1):
        part, pc = ru.host_reset(exe, robot12, p.but(id0=p.id0 + s * n), rows[s * n:(s + 1) * n], count[s * n:(s + 1) * n])
        assert np.array_equal(ru.bits(part), ru.bits(whole[s * n:(s + 1) * n])) and np.array_equal(pc, wc[s * n:(s + 1) * n])


@pytest.mark.parametrize("robot12", [0, 1])
@pytest.mark.parametrize("clearance", [0.0, 0.02])
def test_placing_against_the_oracle(exe, robot12, clearance):
    """the lowest support point of the OUTPUT row, by the oracle, lies at the clearance: rows that start above and below the ground"""
    rows = ru.batch(robot12, 40)
    before = np.array([ru.support_z(robot12, r).min() for r in rows])
    assert (before > 0.05).sum() >= 5 and (before < -0.05).sum() >= 5, "rows on both sides of the ground"
    for p in (ru.full(robot12, clearance=clearance), ru.Params(seed=11, place_on_ground=1, clearance=clearance)):
        out, _ = ru.host_reset(exe, robot12, p, rows, np.zeros(40, np.uint32))
        zmin = np.array([ru.support_z(robot12, r).min() for r in out])
        print("robot12=%d clearance=%g: max |zmin - clearance| %.3e" % (robot12, clearance, np.abs(zmin - clearance).max()))
        assert np.abs(zmin - clearance).max() <= ru.TOL_PLACE
        assert np.array_equal(ru.bits(out[:, :2]), ru.bits(rows[:, :2])), "pos.x and pos.y are never written"


@pytest.mark.parametrize("robot12", [0, 1])
def test_non_finite_members_stay_in_their_row(exe, robot12):
    """NaN and +-Inf in each staged member: every other row comes out as it does without them, and the row's own finite draws that do
    not depend on the member are still bitwise"""
    nq = 12 if robot12 else 8
    base = ru.batch(robot12, 12)
    p = ru.full(robot12)
    clean = ru.reference(robot12, p, base, np.zeros(12, np.uint32))
    members = [W("pos"), W("pos") + 2, W("quat") + 1, W("lin_vel"), W("ang_vel") + 2, W("q"), W("q") + nq - 1, W("qd") + 3]
    for v in (float("nan"), float("inf"), float("-inf")):
        rows = base.copy()
        bad = np.zeros(12, bool)
        for i, w in enumerate(members):
            rows[1 + i, w] = v
            bad[1 + i] = True
        out, cnt = ru.host_reset(exe, robot12, p, rows, np.zeros(12, np.uint32))
        ru.check(out, cnt, clean[0], clean[1], rows, live=~bad, what=repr(v))
        assert np.isfinite(out[~bad][:, :ru.HEAD_WORDS]).all()
        assert (cnt == 1).all()
        for i, w in enumerate(members):                    # the member itself, or what is derived from it, is not finite afterwards
            r = out[1 + i]
            if w in (W("q"), W("q") + nq - 1):
                assert abs(r[w]) == 1.0 or not np.isfinite(r[w])      # (fmax / fmin: a NaN angle comes out as -joint_limit, +-Inf at the clamp)
            else:
                assert not np.isfinite(r[:ru.HEAD_WORDS]).all(), (v, w)


def test_refusals(exe):
    rows = ru.batch(1, 2)
    z = np.zeros(2, np.uint32)
    ok = ru.full(1)
    assert ru.host_reset(exe, 1, ok, rows, z, check_params=True) is not None
    assert ru.host_reset(exe, 1, ok.but(yaw=math.pi, roll=math.pi, pitch=math.pi), rows, z, check_params=True) is not None
    bad = [("yaw", np.nextafter(math.pi, 4.0)), ("roll", 3.2), ("pitch", 4.0), ("yaw", -0.1), ("roll", float("nan")), ("pitch", float("inf")),
           ("clearance", -0.01), ("clearance", float("nan")), ("clearance", float("inf")), ("joint_limit", -1.0), ("joint_limit", float("nan"))]
    for key in ("joint_pos", "joint_vel"):
        for j in (0, 11):
            for v in (-0.1, float("nan"), float("inf")):
                w = list(getattr(ok, key))
                w[j] = v
                bad.append((key, w))
    for key in ("lin_vel", "ang_vel"):
        for k in (0, 2):
            for v in (-1.0, float("nan"), float("-inf")):
                w = list(getattr(ok, key))
                w[k] = v
                bad.append((key, w))
    for key, v in bad:
        assert ru.host_reset(exe, 1, ok.but(**{key: v}), rows, z, check_params=True) is None, (key, v)


def test_sanitized_run(tmp_path):
    """the same program once under AddressSanitizer and UBSan, as a child process: every row and array is a heap block of its exact size"""
    exe = build_host("reset_random_main", san_flags("reset_random_main"), tmp_path)
    for robot12 in (0, 1):
        rows = ru.batch(robot12, 14)
        rows[3, W("q")] = float("nan")
        rows[4, W("quat")] = float("inf")
        mask = (np.arange(14) % 4 != 2).astype(np.uint8)
        got = ru.host_reset(exe, robot12, ru.full(robot12), rows, np.arange(14, dtype=np.uint32), mask)
        live = np.ones(14, bool)
        live[3:5] = False
        want = ru.reference(robot12, ru.full(robot12), rows, np.arange(14, dtype=np.uint32), mask, live)
        ru.check(got[0], got[1], want[0], want[1], rows, mask, live, "sanitized")
