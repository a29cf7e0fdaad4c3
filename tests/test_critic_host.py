"""solorl_critic_obs on the CPU: csrc/critic_obs.hpp -- the per-env arithmetic the HIP kernel runs, one lane per env -- compiled alone by
g++ into a stand-alone program (tests/host/critic_main.cpp) and compared, for both robots, with a numpy restatement of the word table of
include/solorl.h (tests/critic_util.py, whose docstring says which words are held bit for bit and which to the kinematics rows'
tolerance).  Inputs: 64 + 2 rows of the seeded states of tests/kin_util.py.  The test first asserts that these inputs spread over
contact counts, latencies and both signs of the mean gain error.  The same program is built with AddressSanitizer and UBSan and run once
as a child process.  tests/test_critic_gpu.py holds the kernel to the same table."""
import numpy as np
import pytest

from solorl_amd.critic_obs import make_params
from tests import critic_util as cu

ROBOTS = (0, 1)


def _run(c, flags=cu.F_ALL, mask=None, params=None, obs=None, rows=None, fill=None, sanitize=False):
    return cu.run_critic_main(c.cfg, params or c.params, c.rows if rows is None else rows, c.obs if obs is None else obs, c.cmd, c.act, c.kick,
                              c.fill if fill is None else fill, flags, mask, sanitize)


@pytest.mark.parametrize("robot", ROBOTS)
def test_inputs_spread_over_what_the_words_report(robot):
    """If the seed does not give that, change tests/critic_util.py SEED, not this."""
    c = cu.case(robot)
    assert c.n == 66
    _, raw = cu.case_reference(c)
    assert len(np.unique(raw[:, 16])) >= 4
    assert set(raw[:, 17].astype(int)) == {0, 1, 2, 3, 4}
    assert (raw[:, 18] > 0.05).any() and (raw[:, 18] < -0.05).any()
    assert raw[0, 15] == 0 and raw[1, 15] == c.cfg.episode_length
    assert (raw[:, 0:4] > 0).any() and (raw[:, 0:4] == 0).any() and (raw[:, 8:12] > 0).all()
    assert (raw[::5, 19] == 0).all() and (raw[1::5, 19] > 0).all()
    # the default scale of the time step: the last step of an episode reads 1
    want, _ = cu.case_reference(c)
    assert want[1, c.E + 15] == np.float32(1.0) and want[0, c.E + 15] == 0.0


@pytest.mark.parametrize("robot", ROBOTS)
def test_host_program_against_the_numpy_word_table(robot):
    c = cu.case(robot)
    want, raw = cu.case_reference(c)
    got = _run(c)
    cu.check(got, want, raw, cu.scale_of(c.params), c.E)
    # the NaNs with their payloads and the -0.0 of obs_in came through (check compared bits; this says the inputs held them)
    assert cu.bits(got)[2, c.E - 1] == 0x7FC12345 and cu.bits(got)[3, 0] == 0xFFA00001 and cu.bits(got)[4, c.E // 2] == 0x80000000


@pytest.mark.parametrize("robot", ROBOTS)
def test_every_optional_block_absent(robot):
    c = cu.case(robot)
    for flags in (0, cu.F_CMD, cu.F_ACT, cu.F_KICK):
        want, raw = cu.case_reference(c, flags=flags)
        got = _run(c, flags=flags)
        cu.check(got, want, raw, cu.scale_of(c.params), c.E)
        if not flags & cu.F_CMD:
            assert not got[:, c.E + 12:c.E + 15].any()
        if not flags & cu.F_ACT:
            assert not got[:, c.E + 17:c.E + 19].any()
        if not flags & cu.F_KICK:
            assert not got[:, c.E + 19].any()


@pytest.mark.parametrize("robot", ROBOTS)
def test_masked_rows_keep_the_poison(robot):
    """Masked rows keep every byte of critic_out, whatever their inputs hold (NaN here)"""
    c = cu.case(robot)
    mask = (np.arange(c.n) % 3 != 1).astype(np.uint8) * 7
    off = mask == 0
    rows, obs = c.rows.copy(), c.obs.copy()
    rows[off] = np.nan
    obs[off] = np.nan
    want, raw = cu.case_reference(c, mask=mask)
    got = cu.run_critic_main(c.cfg, c.params, rows, obs, c.cmd, c.act, c.kick, c.fill, cu.F_ALL, mask)
    cu.check(got, want, raw, cu.scale_of(c.params), c.E, mask=mask)
    assert (cu.bits(got)[off] == 0xA5A5A5A5).all()


@pytest.mark.parametrize("robot", ROBOTS)
def test_zero_scales_and_overrides(robot):
    c = cu.case(robot)
    zero = make_params(c.cfg, c.E, **{g: 0.0 for g in cu.GROUPS})
    got = _run(c, params=zero)
    assert not got[:, c.E:].any() and (cu.bits(got)[:, :c.E] == cu.bits(c.obs)).all()
    want, raw = cu.case_reference(c, params=zero)
    cu.check(got, want, raw, cu.scale_of(zero), c.E)          # (the sign of a zero too, where the word is held bit for bit)
    other = make_params(c.cfg, c.E, foot_force=[0.01, -0.02, 0.03, 0.04], command=-3.0, time=1.0, gain=100.0)
    want, raw = cu.case_reference(c, params=other)
    cu.check(_run(c, params=other), want, raw, cu.scale_of(other), c.E)


@pytest.mark.parametrize("robot", ROBOTS)
def test_under_the_sanitizers(robot):
    """No sanitizer report (exit 0 with -fno-sanitize-recover=all), with a row of NaN and Inf members among the others; the sanitizer
    build computes what the plain one does; the other rows are bit for bit what they are without the bad row."""
    if cu.critic_main(sanitize=True) is None:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    c = cu.case(robot)
    clean = _run(c, sanitize=True)
    assert (cu.bits(clean) == cu.bits(_run(c))).all()
    rows = c.rows.copy()
    live = 5
    for name, k, v in (("pos", 1, "nan"), ("quat", 2, "inf"), ("q", c.cfg.n_joints - 1, "nan"), ("qd", 0, "-inf"), ("lin_vel", 0, "inf")):
        rows[live, cu.su.SW[name] + k] = float(v)
    cu.su.contact_masks(rows)[live] = 0xFFFFFF
    got = _run(c, rows=rows, sanitize=True)
    keep = np.arange(c.n) != live
    assert (cu.bits(got)[keep] == cu.bits(clean)[keep]).all()
    assert not np.isfinite(got[live, c.E:c.E + 12]).all()
    assert (cu.bits(got)[live, c.E + 12:] == cu.bits(clean)[live, c.E + 12:])[[0, 1, 2, 3, 5, 6, 7]].all()      # words that do not read the pose
