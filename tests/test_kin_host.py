"""solorl_kinematics on the CPU: csrc/kinematics.hpp -- the per-env function the HIP kernel runs, one lane per env -- compiled by g++
into a stand-alone program (tests/host/rows_main.cpp) and compared, for both robots and both inertia rules, on 32 random poses and 32
states of oracle rollouts with contacts, three ways (tests/kin_util.py check_rows):
  1. prim_point against the oracle's prim_points;
  2. kinetic, potential, lin_mom, ang_mom against the oracle's energy_momentum of the same state;
  3. link_pos, link_quat (as rotation matrices), link_com against a numpy forward kinematics written from solorl_amd/models/*.json;
     prim_vel, link_com_vel (and link_ang_vel) against central differences of it, h = 1e-6, 1e-6 relative.
Everything else to |err| <= 1e-10 max(1, |value|).  No sample is left out: the seed is checked to have no foot whose two best profile
rings tie.  The same program is built with AddressSanitizer and UBSan and run once as a child process, with a row of NaN and Inf
members among the others.  tests/test_kin_gpu.py holds the kernel to this program's rows."""
import numpy as np
import pytest

from solorl_amd.config import EnvState
from tests import kin_util as ku
from tests.util import clone


@pytest.mark.parametrize("robot,urdf", ku.CASES)
def test_seeded_samples_have_no_tied_foot_rings(robot, urdf):
    _, states = ku.inputs(robot, urdf)
    gap = ku.foot_ring_gaps(robot, states)
    assert gap > 1e-12, "two foot rings tie to %g in a seeded sample: change tests/kin_util.py SEED" % gap
    # the rollout half really has contacts, with forces
    assert all(s.contact_mask & 0xFFFFFF for s in states[32:])
    assert any(s.lambda_prev[p] > 0 and (s.contact_mask >> p) & 1 for s in states[32:] for p in range(24))


@pytest.mark.parametrize("robot,urdf", ku.CASES)
def test_host_rows_against_oracle_and_numpy_fk(robot, urdf):
    cfg, states = ku.inputs(robot, urdf)
    rows = ku.run_kin_main(cfg, states)
    ku.check_rows(robot, cfg, states, rows)


def test_inertia_rule_changes_the_rotational_terms_only():
    """use_urdf_inertia is read: the two rules give different kinetic energy and angular momentum on a turning robot, the same frames"""
    (c0, s0), (c1, _) = ku.inputs(1, 0), ku.inputs(1, 1)
    a, b = ku.run_kin_main(c0, s0[:8]), ku.run_kin_main(c1, s0[:8])
    assert (ku.member(a, "kinetic") != ku.member(b, "kinetic")).all() and (ku.member(a, "ang_mom") != ku.member(b, "ang_mom")).any()
    for name in ("link_pos", "link_quat", "link_com", "link_com_vel", "prim_point", "prim_vel", "prim_force", "lin_mom", "potential"):
        assert (ku.member(a, name) == ku.member(b, name)).all(), name


def _poisoned(s, nq):
    p = clone(s)
    p.pos[1] = float("nan"); p.quat[2] = float("inf"); p.q[nq - 1] = float("nan"); p.qd[0] = float("-inf")
    p.lin_vel[0] = float("inf"); p.lambda_prev[13] = float("nan"); p.contact_mask = 0xFFFFFF
    return p


@pytest.mark.parametrize("robot", (0, 1))
def test_nonfinite_row_under_the_sanitizers(robot):
    """A row with NaN and Inf members: no sanitizer report (exit 0 with -fno-sanitize-recover=all), non-finite outputs in that row,
    the other rows bit for bit what they are without it."""
    if ku.kin_main(sanitize=True) is None:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    cfg, states = ku.inputs(robot, 1)
    clean = ku.run_kin_main(cfg, states, sanitize=True)
    mixed = list(states)
    mixed[5] = _poisoned(states[5], cfg.n_joints)
    rows = ku.run_kin_main(cfg, mixed, sanitize=True)
    keep = np.arange(len(states)) != 5
    assert (rows[keep].view(np.int64) == clean[keep].view(np.int64)).all()
    assert not np.isfinite(ku.member(rows, "link_pos")[5]).all() and not np.isfinite(ku.member(rows, "kinetic")[5])
    # the sanitizer build computes what the plain one does
    plain = ku.run_kin_main(cfg, states)
    assert ku.close(clean, plain, ku.TOL).all()
