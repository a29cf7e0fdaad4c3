"""The state bank of tests/strata_util.py is fit for its purpose, its yardstick is consistent with itself, and the host build of the
engine's physics source (tests/host/libharness.so: dynamics.hpp in lane mode, compiled by g++) passes it -- all on the CPU, with the
oracle as the only reference.  tests/test_strata_gpu.py holds the kernels to the same bank.

Measured here (figures of the host build in tests/golden/strata_measured.json under host/, of the oracle's twins under oracle/):
  * census: every named stratum and every primitive has 115 samples or more (Solo8: 143), the strip 690; no knife-edge sample;
  * the 1e-15 twin: 0 samples above max(1e-12, s_12) on either robot; the 2^-24 twin: rho p50 / p90 / p99 = 0.72 / 1.29 / 2.2
    (Solo12) and 0.74 / 1.29 / 2.7 (Solo8);
  * the host build at sub-step level: fp64 0 samples above max(1e-12, s_12) and equal masks in all 2048 of either robot;
    fp32 rho 1.2 / 5.7 / 25 (Solo12) and 1.0 / 6.4 / 25 (Solo8) over the whole bank, 0.3 % of it above max(1e-4, 30 s_24)."""
import ctypes as C

import numpy as np
import pytest

from tests import strata_util as su
from tests.host import harness_py

CASES = list(su.ROBOTS)


@pytest.mark.parametrize("name", CASES)
def test_census(name):
    """every stratum the GPU test judges is populated: the random pool alone would leave 'limit rows 3' with a handful"""
    robot = su.ROBOTS[name]
    b, ref = su.bank(robot), su.reference(robot)
    assert b.N <= su.BANK_MAX and b.actions.shape == (b.N, b.n) and b.actions.dtype == np.float32 and np.abs(b.actions).max() <= 1.0
    cont = b.rows[:, :su.N_CONT]
    assert np.isfinite(cont).all() and np.array_equal(cont, cont.astype(np.float32).astype(np.float64))      # float32-representable
    assert not su.col(b.rows, "need_reset").any()
    for k, sel in ref.strata.items():
        need = su.MIN_PRIM if k.startswith("primitive") else su.MIN_STRIP if k == "strip" else su.MIN_STRATUM
        print("census[%s] %-18s %5d" % (name, k, sel.sum()))
        assert sel.sum() >= need, (name, k, int(sel.sum()), need)
    assert len(ref.strata) == 20 + su.nprims(robot) + (robot == su.ROBOT_SOLO8) and su.nprims(robot) == (24 if robot == su.ROBOT_SOLO12 else 20)
    # the strata the existing suite already polices, on which the GPU margin is calibrated
    assert ref.calibration.sum() >= 300, ref.calibration.sum()
    # the drops from 1 m are there: free flight well above the ground
    assert (ref.strata["free flight"] & (su.col(b.rows, "pos")[:, 2] > 0.5)).sum() >= 20
    su.check_knife_edge(ref)
    # the same bank built a second time: seeded, so the GPU run judges the states this run judged
    if name == "solo8":
        saved = su._BANKS.pop(robot)
        try:
            again = su.bank(robot)
            assert np.array_equal(again.rows.view(np.int64), saved.rows.view(np.int64)) and np.array_equal(again.actions, saved.actions)
        finally:
            su._BANKS[robot] = saved


@pytest.mark.parametrize("name", CASES)
def test_yardstick_against_itself(name):
    """The reference alone: a fourth twin at 1e-15 stands in for a correct fp64 implementation and must pass criterion F64 (its
    per-sample bound and exception cap; equal masks); a fifth at 2^-24 gives the rho a single rounding of the inputs costs, which must
    be uniform over the strata: no stratum's p50, p90 or p99 above twice the whole bank's (measured: at most 1.5 x)."""
    robot = su.ROBOTS[name]
    ref = su.reference(robot)
    rows, _ = su.twin(robot, "step", su.EPS_F64, su.SEED + 4)
    viol = su.check_f64("oracle twin 1e-15 / " + name, ref, rows, median_q=False)
    rows, rew = su.twin(robot, "step", su.EPS_24, su.SEED + 5)
    e, _, _, masks = ref.errors(rows, rew)
    r = su.rho(ref, e)
    whole = su.quantiles(r)
    print("strata[oracle twin 2^-24 / %s]: rho p50 %.2f p90 %.2f p99 %.2f; masks differ in %d" % (name, whole["p50"], whole["p90"], whole["p99"], (masks != ref.mask).sum()))
    su.record("oracle/%s" % name, {"twin_f64_violations": int(viol.sum()), "twin_f32_rho": whole})
    for k, q in su.stratum_quantiles(ref, r).items():
        for p in ("p50", "p90", "p99"):
            assert q[p] <= 2.0 * whole[p], "stratum '%s' (%d samples): %s of the 2^-24 twin's rho %.3g against the whole bank's %.3g" % (k, q["n"], p, q[p], whole[p])
    # the figures the issue measured on its own pools (p50 0.70, p90 1.35, p99 2.5): a bank on which a rounding of the inputs costs
    # several times more or less would not be the same yardstick
    assert 0.35 < whole["p50"] < 1.4 and whole["p90"] < 2.7 and whole["p99"] < 5.0, whole


def _host_substep(b, use_float):
    """tests/host/libharness.so from every bank state under the torque of its action -> rows after one physics sub-step"""
    out = np.array(b.rows)
    tau = np.clip(b.actions.astype(np.float64), -1, 1) * b.cfg.max_torque           # oracle/solo_oracle.c apply_action, torque control
    su.col(out, "tau")[:, :b.n] = tau
    L = harness_py.lib()
    for i in range(b.N):
        L.harness_substep(C.cast(C.c_void_p(out.ctypes.data + i * su.ROW_BYTES), C.POINTER(su.EnvState)), C.byref(b.cfg), int(use_float))
    return out


@pytest.mark.parametrize("name", CASES)
def test_host_build(name):
    """harness_py.substep in fp64 and fp32 against the capped oracle's sub-step, stratified by the sub-step's own counts.  fp64: every
    sample within max(1e-12, s_12), every mask equal.  fp32: masks equal outside knife-edge samples; rho per stratum is printed and
    recorded -- an expectation for the GPU (lane mode runs this very source), not a bound on it."""
    robot = su.ROBOTS[name]
    b, ref = su.bank(robot), su.reference(robot, "substep")
    su.check_knife_edge(ref)
    rows = _host_substep(b, False)
    su.check_f64("host fp64 sub-step / " + name, ref, rows, median_q=True, exceptions=False)
    assert np.array_equal(su.col(rows, "contact_mask"), ref.mask)
    rows = _host_substep(b, True)
    e, eq, _, masks = ref.errors(rows)
    assert np.array_equal(masks[~ref.knife], ref.mask[~ref.knife]), np.flatnonzero((masks != ref.mask) & ~ref.knife)[:8]
    r = su.rho(ref, e)
    above = e > np.maximum(1e-4, 30 * ref.s24)
    out = {"all": dict(su.quantiles(r), above=float(above.mean())), "calibration": dict(su.quantiles(r[ref.calibration]), above=float(above[ref.calibration].mean()))}
    for k, sel in ref.strata.items():
        out[k] = dict(su.quantiles(r[sel]), above=float(above[sel].mean()))
    for k, q in out.items():
        print("strata[host fp32 sub-step / %s] %-18s n %4d  rho p50 %.2f p90 %.2f p99 %.2f  above max(1e-4, 30 s_24) %.2f %%" % (name, k, q["n"], q["p50"], q["p90"], q["p99"], 100 * q["above"]))
    su.record("host/%s" % name, out)
    assert np.isfinite(rows[:, :su.N_CONT]).all()


def test_criteria_name_the_stratum():
    """the criteria against results that are wrong in ONE stratum only: each must fail, and its message must name that stratum and list
    samples of it (contacts 0 ... 8 partition the bank and are checked first, so a fault confined to one of them is reported under its name)"""
    robot = su.ROBOTS["solo12"]
    b, ref = su.bank(robot), su.reference(robot)
    good, good_rew = su.twin(robot, "step", su.EPS_F64, su.SEED + 4)
    su.check_f64("self", ref, good, median_q=False)
    # fp64: 1e-9 rad on one joint of the 7-contact samples
    rows = good.copy()
    su.col(rows, "q")[ref.strata["contacts 7"], 0] += 1e-9
    with pytest.raises(AssertionError, match=r"stratum 'contacts 7': \d+ of \d+ samples above(.|\n)*bank +\d+: contacts found +\d+ solved 7"):
        su.check_f64("self", ref, rows, median_q=False)
    # a contact bit and a strip bit (the int32's sign bit) flipped in one 3-contact sample
    rows = good.copy()
    i = int(np.flatnonzero(ref.strata["contacts 3"])[0])
    su.col(rows, "contact_mask")[i] ^= np.int32(-2 ** 31) | np.int32(1)
    with pytest.raises(AssertionError, match=r"stratum 'contacts 3': contact mask differs(.|\n)*bank +%d: (.|\n)*masks [0-9a-f]{8} / [0-9a-f]{8}" % i):
        su.check_f64("self", ref, rows, median_q=False)
    # fp32: the 2^-24 twin passes under its own whole-bank quantiles; 1e-3 on a joint rate of the 8-contact samples does not
    rows, rew = su.twin(robot, "step", su.EPS_24, su.SEED + 5)
    cal = su.quantiles(su.rho(ref, ref.errors(rows)[0]))
    su.check_f32("self", ref, rows, rew, cal)
    su.col(rows, "qd")[ref.strata["contacts 8"], 1] += 1e-3
    with pytest.raises(AssertionError, match=r"stratum 'contacts 8' \(\d+ samples\): p50 of rho"):
        su.check_f32("self", ref, rows, rew, cal)
    # the reward alone
    rew2 = rew.copy(); rew2[5] += 0.01
    with pytest.raises(AssertionError, match="reward off by more than"):
        su.check_reward("self", ref, good, rew2)
