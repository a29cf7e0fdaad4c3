"""solorl_shape_reward on the CPU: csrc/reward_shape.hpp -- the per-env arithmetic the HIP kernel runs, one lane per env -- compiled by
g++ into a stand-alone program (tests/host/shape_main.cpp) and compared, for both robots, with a numpy restatement of the term table of
include/solorl.h (tests/shape_util.py) that takes the feet's points, velocities and forces from the solorl_kinematics host rows.
Inputs: the 64 seeded states of tests/kin_util.py (32 of them oracle rollout states with contacts), actions U(-1.5, 1.5), random valid
memory rows, random done flags, all weights non-zero.  The test first asserts that these inputs reach every term.  Doubles to
|err| <= 1e-10 max(1, |value|) (fp64 on both sides, sums of at most 24 products), integer members exactly, the reward to one f32 ulp,
done rows and masked rows bit for bit.  The same program is built with AddressSanitizer and UBSan and run once as a child process,
with a row of NaN and Inf members among the others.  tests/test_shape_gpu.py holds the kernel to this program's outputs."""
import numpy as np
import pytest

from tests import shape_util as su

ROBOTS = (0, 1)


@pytest.mark.parametrize("robot", ROBOTS)
def test_inputs_reach_every_term(robot):
    """Over the rows that are evaluated (done == 0): every term non-zero somewhere, a first contact, a collision, a foot force over
    the limit.  If the seed does not give that, change tests/shape_util.py SEED, not this."""
    c = su.case(robot)
    assert 8 <= int(c.done.sum()) <= c.n - 8
    assert all(w != 0.0 for w in c.params.weight)
    (_, _, terms, _), firsts = su.reference(c)
    live = c.done == 0
    for k, name in enumerate(su.TERMS):
        assert (terms[live, k] != 0.0).any(), name
    assert firsts[live].any()
    assert (terms[live, su.TERMS.index("collision")] >= 1).any()
    assert (terms[live, su.TERMS.index("foot_force")] > 0).any()
    assert (terms[live, su.TERMS.index("feet_air_time")] != 0).any()


@pytest.mark.parametrize("robot", ROBOTS)
def test_host_program_against_the_numpy_term_table(robot):
    c = su.case(robot)
    want, _ = su.reference(c)
    su.check_outputs(c, su.run_shape_main(c), want)


@pytest.mark.parametrize("robot", ROBOTS)
def test_masked_rows_and_absent_arrays(robot):
    """Masked rows keep every byte, whatever they hold (NaN and 0xA5 bytes here, in the inputs and in the outputs); every optional
    array absent once."""
    c = su.case(robot)
    mask = (np.arange(c.n) % 3 != 1).astype(np.uint8) * 7
    for poison in (np.float64("nan"), np.frombuffer(b"\xa5" * 8, np.float64)[0]):
        p = su.types.SimpleNamespace(**vars(c))
        p.states, p.mem, p.terms, p.ep = (a.copy() for a in (c.states, c.mem, c.terms, c.ep))
        p.reward, p.actions = c.reward.copy(), c.actions.copy()
        off = mask == 0
        p.states[off] = poison; p.mem[off] = poison; p.terms[off] = poison; p.ep[:, off] = poison
        p.reward[off] = np.float32(poison) if np.isnan(poison) else np.frombuffer(b"\xa5" * 4, np.float32)[0]
        p.actions[off] = np.float32("nan")
        want, _ = su.reference(p, mask=mask)
        su.check_outputs(p, su.run_shape_main(p, mask=mask), want, mask=mask)
    for absent in (su.F_DONE, su.F_REWARD, su.F_TERMS, su.F_EP):
        flags = su.F_ALL & ~absent
        want, _ = su.reference(c, flags=flags)
        su.check_outputs(c, su.run_shape_main(c, flags=flags), want, flags=flags)


@pytest.mark.parametrize("robot", ROBOTS)
def test_nonfinite_row_under_the_sanitizers(robot):
    """A row with NaN and Inf members: no sanitizer report (exit 0 with -fno-sanitize-recover=all), the other rows bit for bit what
    they are without it."""
    if su.shape_main(sanitize=True) is None:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    c = su.case(robot)
    live = int(np.nonzero(c.done == 0)[0][2])
    clean = su.run_shape_main(c, sanitize=True)
    rows = c.states.copy()
    nq = c.cfg.n_joints
    for name, k, v in (("pos", 1, "nan"), ("quat", 2, "inf"), ("q", nq - 1, "nan"), ("qd", 0, "-inf"), ("lin_vel", 0, "inf"), ("tau", 1, "nan"),
                       ("lambda_prev", 13, "nan")):
        rows[live, su.SW[name] + k] = float(v)
    su.contact_masks(rows)[live] = 0xFFFFFF
    got = su.run_shape_main(c, states=rows, sanitize=True)
    keep = np.arange(c.n) != live
    for g, w in zip(got, clean):
        if g.shape[0] == c.n:
            assert (su.bits(g).reshape(c.n, -1)[keep] == su.bits(w).reshape(c.n, -1)[keep]).all()
        else:
            assert (su.bits(g).reshape(su.EP_FIELDS, c.n, 8)[:, keep] == su.bits(w).reshape(su.EP_FIELDS, c.n, 8)[:, keep]).all()
    assert not np.isfinite(got[2][live]).all() and not np.isfinite(got[1][live])
    # the sanitizer build computes what the plain one does
    plain = su.run_shape_main(c)
    for g, w in zip(clean, plain):
        assert su.ku.close(g, w, su.ku.TOL).all()
