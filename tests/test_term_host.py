"""Early termination (include/solorl.h solorl_terminate) without a GPU.

The row arithmetic of the kernel is solorl_amd/csrc/termination.hpp, plain host-and-device functions: tests/host/terminate_main.cpp
compiles them alone with g++ (no -march=native, contraction off) and its arrays are compared bitwise with tests/term_util.py, the
header's table in numpy, on crafted rows: each rule just below, at and just above its threshold, several rules at once, min_steps,
rows that are done on entry, masked rows against a poison fill, a Solo8, and NaN and +-Inf in every member that is read.  The same
stand-alone program runs once under AddressSanitizer and UBSan; it is never loaded into python.  One test needs the prediction only:
the crafted rows reach every branch of the table."""
import numpy as np
import pytest

from tests import term_util as tu
from tests.host_util import build_host, san_flags



@pytest.fixture(scope="module")
def exe():
    return build_host("terminate_main")


def run_cases(exe, robot12, p, mask=None, info=True, stats=True, n=None):
    n = len(tu.cases(robot12)) if n is None else n
    rows, done, reward, names = tu.batch(robot12, n)
    before = tu.Arrays(n, done, reward, seed=n)
    got = tu.host_terminate(exe, robot12, p, tu.SIM_DT, rows, before, mask, info, stats)
    want = tu.reference(robot12, p, tu.SIM_DT, rows, before, mask, info, stats)
    assert tu.same(got, want) == [], (tu.same(got, want), [names[i] for i in np.nonzero(got.fired != want.fired)[0]])
    return before, want, names


@pytest.mark.parametrize("robot12", (True, False))
def test_host_rows_equal_the_table(exe, robot12):
    p = tu.params(robot12)
    before, after, names = run_cases(exe, robot12, p)
    assert after.done.sum() > before.done.astype(bool).sum() and (after.fired == tu.ALL).any()
    # a single rule enabled: the others' thresholds are not looked at
    for bit in (tu.HEIGHT, tu.TILT, tu.CONTACT, tu.JOINT):
        _, one, _ = run_cases(exe, robot12, p.but(rules=bit))
        assert set(np.unique(one.fired)) == {0, bit}
    # no min_steps, another terminal reward, a force threshold of 0
    _, early, _ = run_cases(exe, robot12, p.but(min_steps=0, terminal_reward=-2.5, contact_force_min=0.0))
    assert early.fired[names.index("fallen at timestep 0")] == tu.HEIGHT and np.float32(-2.5) in early.reward


@pytest.mark.parametrize("robot12", (True, False))
def test_masked_rows_keep_the_poison_and_null_blocks_are_skipped(exe, robot12):
    p = tu.params(robot12)
    n = len(tu.cases(robot12))
    mask = (np.arange(n) % 3 != 1)
    before, after, _ = run_cases(exe, robot12, p, mask=mask)
    for k, v in after.bits().items():
        assert np.array_equal(v[..., ~mask], before.bits()[k][..., ~mask]), k        # fired: the poison; the sums: what they held
    assert np.all(after.fired[~mask] == tu.POISON8) and np.all(after.fired[mask] != tu.POISON8)
    # rows where nothing fires write fired_out and nothing else
    quiet = mask & (after.fired == 0)
    for k in ("done", "reward", "timeout", "success", "ep_reward", "ep_stats", "stats"):
        assert np.array_equal(after.bits()[k][..., quiet], before.bits()[k][..., quiet]), k
    assert np.all(after.timeout[quiet] == tu.POISON8)
    run_cases(exe, robot12, p, info=False)
    run_cases(exe, robot12, p, stats=False, mask=mask)
    run_cases(exe, robot12, p, info=False, stats=False)


def test_a_solo8_ignores_joints_8_to_11_and_primitives_20_to_23(exe):
    """The entry point refuses contact_prims 20..23 on a Solo8; the row arithmetic masks them all the same, and a Solo12 reads them"""
    rows, done, reward, names = tu.batch(False, len(tu.cases(False)))
    i = names.index("contact of a shoulder that is not chosen")
    p = tu.params(False).but(contact_prims=tu.params(False).contact_prims | (0xF << 20))
    arr = tu.Arrays(len(names), done, reward)
    got8 = tu.host_terminate(exe, False, p, tu.SIM_DT, rows, arr)
    assert tu.same(got8, tu.reference(False, p, tu.SIM_DT, rows, arr)) == [] and got8.fired[i] == 0
    assert got8.fired[names.index("joint 8 of a Solo8")] == 0 and got8.fired[names.index("joint 11 of a Solo8")] == 0
    p12 = p.but(joint_lo=[tu.LO] * 12, joint_hi=[tu.HI] * 12)
    got12 = tu.host_terminate(exe, True, p12, tu.SIM_DT, rows, arr)
    assert tu.same(got12, tu.reference(True, p12, tu.SIM_DT, rows, arr)) == []
    assert got12.fired[i] == tu.CONTACT and got12.fired[names.index("joint 8 of a Solo8")] == tu.JOINT
    assert tu.host_terminate(exe, False, p, tu.SIM_DT, rows, arr, check=True) is None          # ... and the parameters are refused
    assert tu.host_terminate(exe, True, p12, tu.SIM_DT, rows, arr, check=True) is not None


def test_boundary_shapes_under_the_sanitizers(tmp_path):
    """The same stand-alone program with AddressSanitizer and UBSan on n = 1 and on every crafted row of both robots (every array and
    every state row is a heap block of exactly its size: an access past one ends the run)"""
    san = build_host("terminate_main", san_flags("terminate_main"), tmp_path)
    for robot12 in (True, False):
        p = tu.params(robot12)
        run_cases(san, robot12, p, n=1)
        run_cases(san, robot12, p, mask=np.arange(len(tu.cases(robot12))) % 2 == 0)
        run_cases(san, robot12, p, info=False, stats=False)


def test_the_cases_reach_every_branch_of_the_table():
    """From the prediction alone: what each crafted row is named after is what the table gives for it"""
    for robot12 in (True, False):
        p = tu.params(robot12)
        cs = tu.cases(robot12)
        seen = set()
        for name, row, done, expect in cs:
            f = 0 if done else tu.fired_bits(robot12, p, tu.SIM_DT, row)          # (a row that is done on entry is not looked at)
            assert f == expect, (robot12, name, f, expect)
            seen.add(f)
        assert {0, tu.HEIGHT, tu.TILT, tu.CONTACT, tu.JOINT, tu.ALL} <= seen
        assert any(done for _, _, done, _ in cs) and len(cs) <= 130
    # the thresholds are reached exactly: one ulp decides
    edge = tu._force_edge(5.0, tu.SIM_DT)
    assert edge / tu.SIM_DT >= 5.0 > np.nextafter(edge, 0.0) / tu.SIM_DT
    up = lambda qx: 1.0 - 2.0 * (qx * qx + 0.0)
    assert up(0.5) == 0.5 and up(np.nextafter(0.5, 1.0)) < 0.5 < up(np.nextafter(0.5, 0.0))
