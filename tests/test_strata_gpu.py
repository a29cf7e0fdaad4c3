"""Every instantiation of the step kernel against the fp64 oracle PER STRATUM, fallen robots included: the bank, the strata and the
yardstick of tests/strata_util.py (made with the oracle alone; tests/test_strata_cpu.py checks them and the host build of the same
source), one control step from every bank state in one launch per mode.

The resynced parity tests of tests/test_parity_gpu*.py step a random policy from the reset crouch and the fall rule resets what falls
over: 1.5 % of their samples have five contacts or more, and those are judged by whole-sample quantiles.  Here every number of solved
contacts 0..8, the contact cap binding, 0..4 joint-limit rows (rows 3 and 4 take contact slots), more limit candidates than rows, a
base upright / on its side / inverted, free flight, every collision primitive in contact and the treadmill strip each have 100
samples or more and are judged on their own.

  * fp64 modes (criterion F64): per sample e <= max(1e-12, s_12) -- what a 1e-12 relative change of the start state does to the oracle
    itself -- with at most 0.5 % of a stratum (1 sample below 200) excepted; masks and strip bits equal outside knife-edge samples; the
    per-stratum median of e on q below 1e-13.
  * fp32 modes (criterion F32): rho = e / max(s_24, 1e-7) per stratum within PARITY_MARGIN x the quantiles MEASURED on the MI355X in mode
    f32-team-helper on the calibration strata (upright, at most 4 solved contacts, at most 1 limit row: what the rest of the suite
    polices) -- tests/golden/strata_measured.json, gpu/calibration; no unexplained sample above 1e-3 rad, masks, reward."""
import numpy as np
import pytest
import torch

from solorl_amd.config import PRECISION_F64
from tests import strata_util as su

pytestmark = pytest.mark.gpu

#        mode              f64  environment                                          properties of the handle
MODES = {"f64-team":        (1, {"SOLORL_TEAM": "1"},                                {"f64": 1, "lanes_per_env": 16}),
         "f64-lane":        (1, {"SOLORL_TEAM": "0"},                                {"f64": 1, "lanes_per_env": 1}),
         "f32-team-helper": (0, {"SOLORL_TEAM": "1", "SOLORL_HELPER_WAVE": "1"},     {"f64": 0, "lanes_per_env": 16, "helper_wave": 1}),
         "f32-team-classic": (0, {"SOLORL_TEAM": "1", "SOLORL_HELPER_WAVE": "0"},    {"f64": 0, "lanes_per_env": 16, "helper_wave": 0}),
         "f32-lane":        (0, {"SOLORL_TEAM": "0"},                                {"f64": 0, "lanes_per_env": 1, "helper_wave": 0})}
CALIBRATION_MODE = "f32-team-helper"


def _engine_step(monkeypatch, b, mode):
    """a handle of the bank's size in `mode`: reset, ONE set_states of every member group, one step_inplace, one get_states
    -> (rows after [N, ROW_WORDS] float64, rewards [N])"""
    from solorl_amd.state import StateBatch
    from solorl_amd.vec_env import SoloVecEnv
    f64, environ, props = MODES[mode]
    cfg = b.cfg.copy()
    if f64:
        cfg.precision = PRECISION_F64
    for k in ("SOLORL_TEAM", "SOLORL_HELPER_WAVE", "SOLORL_SORT", "SOLORL_PGS_PIPE", "SOLORL_SPREAD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in environ.items():
        monkeypatch.setenv(k, v)                     # (read at solorl_create)
    env = SoloVecEnv(cfg, b.N, device=torch.device("cuda:0"), seed=1)
    for k, v in props.items():
        assert env.get_property(k) == v, (mode, k, env.get_property(k))
    env.reset()
    env.set_states(StateBatch(data=torch.from_numpy(np.array(b.rows)).to("cuda:0")))
    _, rew, done, info = env.step_inplace(torch.from_numpy(np.array(b.actions)).to("cuda:0"))
    rows = env.get_states().data.cpu().numpy()
    rew = rew.double().cpu().numpy().reshape(-1)
    assert not done.any().item() and info["nan_reset"].sum().item() == 0
    env.close()
    return rows, rew


@pytest.mark.parametrize("name", list(su.ROBOTS))
@pytest.mark.parametrize("mode", list(MODES))
def test_strata_vs_oracle(gpu_device, monkeypatch, mode, name):
    robot = su.ROBOTS[name]
    b, ref = su.bank(robot), su.reference(robot)
    label = "%s / %s" % (mode, name)
    rows, rew = _engine_step(monkeypatch, b, mode)
    assert np.isfinite(rows[:, :su.N_CONT]).all() and np.isfinite(rew).all()
    su.check_knife_edge(ref)
    e, _, _, _ = ref.errors(rows)
    if MODES[mode][0]:
        su.check_f64(label, ref, rows)
        su.check_reward(label, ref, rows, rew)
        su.record("gpu/%s/%s" % (mode, name), {"e": su.quantiles(e), "violations": int((e > np.maximum(1e-12, ref.s12)).sum())})
        return
    r = su.rho(ref, e)
    cal = su.quantiles(r[ref.calibration])
    print("strata[%s]: rho on the calibration strata (n %d) p50 %.3g p90 %.3g p99 %.3g; whole bank p50 %.3g p90 %.3g p99 %.3g" % (
        label, cal["n"], cal["p50"], cal["p90"], cal["p99"], *(su.quantiles(r)[k] for k in ("p50", "p90", "p99"))))
    for k, q in su.stratum_quantiles(ref, r).items():
        print("strata[%s] %-18s n %4d  rho p50 %.3g p90 %.3g p99 %.3g" % (label, k, q["n"], q["p50"], q["p90"], q["p99"]))
    su.record("gpu/%s/%s" % (mode, name), dict(su.stratum_quantiles(ref, r), all=su.quantiles(r), calibration=cal))
    if mode == CALIBRATION_MODE:
        su.record("gpu/calibration/%s" % name, cal)
    measured = su.measured("gpu/calibration/%s" % name)
    assert measured is not None, ("no calibration quantiles for %s in tests/golden/strata_measured.json: run this test's %s case on the MI355X and copy "
                                  "what it wrote to strata_stats.json ($SOLORL_STATS_DIR, or build/strata) with tools/dev/collect_strata_stats.py (measured now in this mode: %s)" % (
                                      name, CALIBRATION_MODE, cal))
    su.check_f32(label, ref, rows, rew, measured)
