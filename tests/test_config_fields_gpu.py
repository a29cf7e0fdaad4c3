"""solorl_config fields that no other GPU test moves off their defaults, on the HIP engine against the fp64 oracle running the same value:
the table `CASES` of tests/test_config_fields.py (which also shows, on the oracle alone, that every case moves the compared quantity by
>= 1e-3 -- ten times the fp32 median bound below, so an instantiation that ignores or hard-codes the field cannot pass).

Every case runs in the three instantiations of the step: team fp32 (the default), lane mode (SOLORL_TEAM=0) and fp64.  Shape: 64 envs, 12
control steps, the oracle reloaded with the engine's state before every step (tests/test_parity_gpu3.py::
test_friction_model_and_contact_erp_options_vs_oracle).  Bounds over the samples of a case:
  fp32: median < 1e-4, p90 < 1e-3, contact-mask mismatches <= 2 % of the samples;    fp64: median < 1e-11, p90 < 1e-7
and, once measured on the MI355X, 3 x the measured quantiles (tests/util.py check_parity_stats, "config_field/<field>_<value>/<mode>").

The kernel FORMS -- the helper-wave kernel, whose barrier count is 2 x frame_skip, and the K-step kernel -- are compared bitwise with
the classic one-step kernel for the fields their control flow reads: frame_skip 2 and 6, hold_torque 1."""
import numpy as np
import pytest
import torch

from solorl_amd.config import PRECISION_F64
from tests.util import check_parity_stats
from tests.test_config_fields import CASES, N_ENVS, N_STEPS, OracleSide, case_config, case_id, obs_diff, run_scenario

pytestmark = pytest.mark.gpu

MODES = ("team", "lane", "f64")


class EngineSide:
    """The HIP engine behind the call shape of tests/test_config_fields.py::OracleSide"""

    def __init__(self, cfg, N, seed):
        from solorl_amd.vec_env import SoloVecEnv
        self.e = SoloVecEnv(cfg, N, device="cuda:0", seed=seed)
        self.cfg, self.N = cfg, N

    def caps(self, contacts, limits):
        assert self.e.get_property("max_contacts") == contacts and self.e.get_property("max_limit_rows") == limits

    def reset(self):
        return self.e.reset().cpu().numpy().astype(np.float64)

    def step(self, a):
        obs, rew, done, _ = self.e.step(torch.from_numpy(np.asarray(a, np.float32)).cuda())
        return obs.cpu().numpy().astype(np.float64), rew.cpu().numpy()[:, 0].astype(np.float64), done.cpu().numpy() != 0

    def get_state(self, i):
        return self.e.get_state(i)

    def set_state(self, i, s):
        self.e.set_state(i, s)


def _sides(monkeypatch, case, mode, seed=3):
    c = case_config(case, True)
    if mode == "f64":
        c.precision = PRECISION_F64
    for k in ("SOLORL_SORT", "SOLORL_TEAM", "SOLORL_HELPER_WAVE"):
        monkeypatch.delenv(k, raising=False)
    if mode == "lane":
        monkeypatch.setenv("SOLORL_TEAM", "0")
    eng = EngineSide(c, N_ENVS, seed)
    monkeypatch.delenv("SOLORL_TEAM", raising=False)
    assert eng.e.get_property("lanes_per_env") == (1 if mode == "lane" else 16) and eng.e.get_property("f64") == (mode == "f64")
    return eng, OracleSide(c, N_ENVS, seed)


# the whole observation is what the history cases compare, and the engine hands it over as float32: no fp64 bound can apply to it
PARAMS = [pytest.param(c, m, id="%s-%s" % (case_id(c), m)) for c in CASES for m in MODES if not (c.scenario == "history" and m == "f64")]


@pytest.mark.parametrize("case,mode", PARAMS)
def test_config_field_vs_oracle(gpu_device, monkeypatch, case, mode):
    eng, orc = _sides(monkeypatch, case, mode)
    r = run_scenario(case, eng, orc, strip_side="follow")
    s, x = np.asarray(r["samples"]), r["extra"]
    f64 = mode == "f64"
    name = "config_field/%s/%s" % (case_id(case), mode)
    q = check_parity_stats(name, s, floor=1e-13 if f64 else 1e-7)
    print("%s: %d samples of %d, contact-mask mismatches %d, %s" % (name, s.size, r["total"], r["mask_mismatch"],
                                                                   {k: v for k, v in x.items() if np.isscalar(v) or k in ("timeouts", "obs_max")}))
    if case.quantity == "reward":
        # |r_engine - r_oracle|: the median bound of tests/test_parity_gpu.py::test_step_matches_oracle_resynced.  The fp64 engine
        # returns its reward as float32 like the fp32 one: half an ulp of a reward of up to 16 in magnitude is 1e-6
        assert q["p50"] < (1e-6 if f64 else 1e-3), q
    elif f64:
        assert q["p50"] < 1e-11 and q["p90"] < 1e-7, q
    else:
        assert q["p50"] < 1e-4 and q["p90"] < 1e-3, q
    assert r["mask_mismatch"] <= 0.02 * r["total"], (r["mask_mismatch"], r["total"])
    sc = case.scenario
    if case.quantity == "joint_angle_on_strip":
        assert s.size > 0.5 * r["total"], (s.size, r["total"])                 # more than half of the samples are on the strip
    elif sc == "reset":
        assert s.size == 2 * N_ENVS
        assert all(x["rng_equal"]) and all(x["side_equal"])                    # the same Philox draws, every env at timestep 0
        assert x["timeouts"] == (N_ENVS, N_ENVS)                               # the second batch of samples is the in-step auto-reset
        assert max(x["obs_max"]) < 2e-3, x["obs_max"]                          # observations: tests/test_parity_gpu.py::test_reset_matches_oracle
        if case.quantity == "treadmill_y":
            assert s.max() < 1e-6 and set(np.round(np.abs(x["treadmill_y"]), 6)) == {case.value}
        if case.quantity == "goal":
            assert s.max() < 2.5e-6                                            # (float32 of a coordinate of up to 6 m)
    elif sc == "history":
        D = eng.cfg.state_dim
        assert eng.e.obs_dim == D * (1 + case.value)
        assert obs_diff(*x["reset_obs"], D).max() < 2e-3
        assert all(x["done_equal"]) and x["resets"][6] == N_ENVS               # the timeout at episode_length = 7 refills the history
    else:
        assert s.size > 0.5 * N_ENVS * N_STEPS
        if sc == "resynced_limits":
            assert x["limit_rows"] > 0.5 * r["total"]
    eng.e.close()


# ------------------------------------------------------------------------------------------------ kernel forms, bitwise
FORM_FIELDS = [("frame_skip", 2), ("frame_skip", 6), ("hold_torque", 1)]


def _form_cfg(field, value, episode_length):
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    c = default_config(ROBOT_SOLO12, TASK_WALK); c.num_history_stack = 1; c.episode_length = episode_length
    setattr(c, field, value)
    return c


@pytest.mark.parametrize("field,value", FORM_FIELDS)
def test_helper_wave_kernel_reads_the_field_bitwise(gpu_device, monkeypatch, field, value):
    """SOLORL_HELPER_WAVE=0 against the default two-wavefront kernel, N = 67, 20 steps: every output of every step, the accumulators and
    every env's state (tests/test_helper_wave_gpu.py).  frame_skip is the helper wavefront's own loop count: a wrong one is a hang or
    a stale collision front, not a rounding difference."""
    from tests.test_helper_wave_gpu import _env, _same_rollout
    cfg = _form_cfg(field, value, 12)
    on, off = _env(monkeypatch, cfg, 67, 1), _env(monkeypatch, cfg, 67, 0)
    assert _same_rollout(on, off, 20) > 0                # episodes ended (timeout at 12) inside the 20 steps
    on.close(); off.close()


@pytest.mark.parametrize("field,value", FORM_FIELDS)
def test_k_step_kernel_reads_the_field_bitwise(gpu_device, monkeypatch, field, value):
    """solorl_step_n(K = 5) against 5 single steps (tests/test_step_n_gpu.py), episode_length = 3: the timeout reset of every env lies
    inside the window."""
    from tests.test_step_n_gpu import _pair, _per_step, _same_state, INFO
    N, K = 67, 5
    ref, cand = _pair(monkeypatch, _form_cfg(field, value, 3), N)
    assert cand.get_property("step_n_one_launch") == 1
    g = torch.Generator(device="cuda:0"); g.manual_seed(11)
    for window in range(2):
        acts = torch.rand(K, N, 12, device="cuda:0", generator=g) * 3 - 1.5
        want = _per_step(ref, acts)
        o, r, d, info = cand.step_n_inplace(acts)
        assert torch.equal(o, want["obs"]) and torch.equal(r, want["rew"]) and torch.equal(d, want["done"]), window
        assert torch.equal(info["applied_torque"], want["applied_torque"])
        for f in INFO:
            assert torch.equal(info[f], want[f]), (window, f)
        assert int(info["timeout"].sum()) > N // 2                               # (timeouts, and the resets behind them, inside the window)
    torch.cuda.synchronize()
    assert torch.equal(ref._ep_stats, cand._ep_stats)
    _same_state(ref, cand, range(N))
    ref.close(); cand.close()
