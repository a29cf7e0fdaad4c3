"""solorl_dynamics on the CPU: csrc/dyn_tensors.hpp -- the per-env function the HIP kernel runs, one lane per env -- compiled by g++
into a stand-alone program (tests/host/rows_main.cpp) and held, for both robots and both inertia rules, on the 32 random poses and 32
oracle rollout states of tests/kin_util.inputs, to the five comparisons of tests/dyn_util.py check_rows:
  1. mass_matrix against the oracle's dense M (|err| <= 1e-10 sqrt(M_aa M_bb)), symmetric to the bit, exact zeros, Cholesky;
  2. bias against the oracle's h at the default damping and at damping 0; gravity against h at rest, (0, 0, m g) and dV/dq;
  3. kinetic energy, momentum, foot velocities and foot points against the host program of solorl_kinematics on the same states;
  4. foot_jac and foot_acc_bias against a numpy restatement, itself checked by second differences of the forward kinematics;
  5. solve(M, tau - bias) against the oracle's forward dynamics.
Everything else to |err| <= 1e-10 max(1, |ref|).  The same program is built with AddressSanitizer and UBSan and run as a child process
with a row of NaN and a row of Inf members among the others.  tests/test_dyn_gpu.py holds the kernel to this program's rows."""
import numpy as np
import pytest

from tests import dyn_util as du
from tests import kin_util as ku
from tests.util import clone


@pytest.mark.parametrize("robot,urdf", ku.CASES)
def test_host_rows_against_oracle_kinematics_and_numpy(robot, urdf):
    cfg, states = ku.inputs(robot, urdf)
    assert cfg.damping == 0.04
    kin = ku.run_kin_main(cfg, states)
    worst = du.check_rows(robot, cfg, states, du.run_dyn_main(cfg, states), kin)
    print("numpy Jdot v against second differences, worst relative error: %.3g" % worst["restatement"])
    cfg0 = du.no_damping(cfg)
    du.check_rows(robot, cfg0, states, du.run_dyn_main(cfg0, states), kin, restatement=False)


def test_damping_and_inertia_rule_are_read():
    """damping changes bias and nothing else; use_urdf_inertia changes M and bias, not the feet"""
    (c0, s0), (c1, _) = ku.inputs(1, 0), ku.inputs(1, 1)
    a, b, c = du.run_dyn_main(c0, s0[:8]), du.run_dyn_main(du.no_damping(c0), s0[:8]), du.run_dyn_main(c1, s0[:8])
    assert (du.member(a, "bias")[:, :18] != du.member(b, "bias")[:, :18]).all()
    for name in ("mass_matrix", "gravity", "foot_jac", "foot_acc_bias", "foot_pos"):
        assert (du.member(a, name) == du.member(b, name)).all(), name
    assert (du.member(a, "mass_matrix")[:, 3:6, 3:6] != du.member(c, "mass_matrix")[:, 3:6, 3:6]).any()
    assert (du.member(a, "mass_matrix")[:, 0:3, :] == du.member(c, "mass_matrix")[:, 0:3, :]).all()        # mass and first moment
    for name in ("gravity", "foot_jac", "foot_acc_bias", "foot_pos"):
        assert (du.member(a, name) == du.member(c, name)).all(), name


def _nan_row(s, nq):
    p = clone(s)
    p.pos[1] = float("nan"); p.quat[2] = float("nan"); p.q[nq - 1] = float("nan"); p.qd[0] = float("nan"); p.ang_vel[2] = float("nan")
    return p


def _inf_row(s, nq):
    p = clone(s)
    p.pos[0] = float("inf"); p.quat[1] = float("-inf"); p.q[0] = float("inf"); p.qd[nq - 1] = float("-inf"); p.lin_vel[0] = float("inf")
    return p


@pytest.mark.parametrize("robot", (0, 1))
def test_nonfinite_rows_under_the_sanitizers(robot):
    """A row with NaN and a row with Inf members, each between good rows: no sanitizer report (exit 0 with -fno-sanitize-recover=all),
    non-finite outputs in those rows, the other rows byte for byte what they are without them."""
    if du.dyn_main(sanitize=True) is None:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    cfg, states = ku.inputs(robot, 1)
    states = states[:8]
    clean = du.run_dyn_main(cfg, states, sanitize=True)
    mixed = list(states)
    mixed[2] = _nan_row(states[2], cfg.n_joints)
    mixed[4] = _inf_row(states[4], cfg.n_joints)
    rows = du.run_dyn_main(cfg, mixed, sanitize=True)
    keep = ~np.isin(np.arange(len(states)), (2, 4))
    assert (rows[keep].view(np.int64) == clean[keep].view(np.int64)).all()
    for bad in (2, 4):
        for name in ("mass_matrix", "bias", "gravity", "foot_jac", "foot_acc_bias", "foot_pos"):
            assert not np.isfinite(du.member(rows, name)[bad]).all(), (bad, name)
    # the sanitizer build computes what the plain one does
    assert ku.close(clean, du.run_dyn_main(cfg, states), ku.TOL).all()
