"""Every field of solorl_config is moved off its default by some test -- and the move matters.

`CASES` is the table of (field, value, scenario, compared quantity) that tests/test_config_fields_gpu.py runs on the HIP engine against the
fp64 oracle running the same value.  A field is copied into the kernel parameters at solorl_create and read by three instantiations of
the step (team fp32, lane, fp64) and by the helper-wave and K-step kernels; one that ignores or hard-codes it changes nothing at the
defaults, which is all the rest of the suite runs.

This module (no GPU) holds the two conditions that make the table worth something:
  * test_every_case_moves_the_oracle: on the oracle alone, the changed value against the default from identical states, over the samples
    the GPU test asserts on: the median of the compared quantity is >= 1e-3 = 10 x the fp32 median bound of the GPU test.  An engine
    that ignores the field sits that far from the oracle and cannot pass.  A condition on the INPUTS, not a measurement of the engine;
  * test_every_config_field_is_exercised: every name of SoloConfig._fields_ is in CASES or in COVERED_ELSEWHERE, whose entries name an
    existing test function that mentions the field.  A field added later without a test fails here.

The scenario code (what states, what actions, which samples) is shared by both modules through two small adapters with one call shape,
`OracleSide` here and the engine's in the GPU module."""
import collections
import importlib
import inspect
import os

import numpy as np
import pytest

from tests.util import state_vec
from solorl_amd.config import (SoloConfig, default_config, ROBOT_SOLO12, TASK_WALK, TASK_POINTGOAL, CONTROL_PD, CONTROL_TORQUE)

Case = collections.namedtuple("Case", "field value scenario quantity")

LYING_HEIGHT = 0.03
N_ENVS, N_STEPS = 64, 12          # envs, resynced control steps per case

CASES = [
    # one control step from identical states, random torques: max joint-angle error per env and step
    Case("frame_skip", 1, "resynced", "joint_angle"),
    Case("frame_skip", 2, "resynced", "joint_angle"),
    Case("frame_skip", 6, "resynced", "joint_angle"),
    Case("hold_torque", 1, "resynced", "joint_angle"),
    Case("sim_dt", 1.0 / 480.0, "resynced", "joint_angle"),
    # a robot on its feet carries gravity through its contacts and its joints hardly move with it within one control step; on its back,
    # the legs in the air, every leg is a pendulum
    Case("gravity", 3.7, "resynced_lying", "joint_angle"),
    Case("damping", 0.5, "resynced", "joint_angle"),
    Case("damping", 0.0, "resynced", "joint_angle"),
    Case("max_velocity", 1.0, "resynced", "joint_angle"),                 # the K5 clamp
    Case("linear_slop", 5e-3, "resynced", "joint_angle"),
    Case("collision_margin", 0.0, "resynced", "joint_angle"),
    Case("collision_margin", 0.005, "resynced", "joint_angle"),
    Case("max_torque", 1.0, "resynced", "joint_angle"),                   # (torque control: the scenario's)
    Case("solver_iterations", 1, "resynced", "joint_angle"),              # (the K7 residual exit stays on: the cap binds before it)
    # pointgoal: the progress term is the travel towards the goal divided by reward_dt
    Case("reward_dt", 1.0 / 240.0, "resynced_pointgoal", "reward"),
    # erp acts on joint-limit rows only, and there are none at +-10 rad: a small joint_limit so that they exist
    Case("erp", 0.8, "resynced_limits", "joint_angle"),
    # the strip: only samples whose (oracle) contact mask has a strip bit (24 + foot) see these two.  PD stance, small actions
    Case("treadmill_friction", 0.1, "treadmill_stance", "joint_angle_on_strip"),
    Case("treadmill_half_width", 0.2, "treadmill_stance_narrow", "joint_angle_on_strip"),
    # these act at reset (the full one and the auto-reset after a short episode)
    Case("treadmill_offset", 0.1, "reset", "treadmill_y"),
    Case(("settle_min", "settle_max"), (0, 0), "reset", "state"),
    Case(("settle_min", "settle_max"), (2, 13), "reset", "state"),
    Case("goal_radius", 5.0, "reset", "goal"),
    # 0 skips the history push; 2 is the boundary between the register-held and the HBM-held levels
    Case("num_history_stack", 0, "history", "observation"),
    Case("num_history_stack", 2, "history", "observation"),
]

# fields that CASES leaves alone: the test that moves each of them off its default
COVERED_ELSEWHERE = {
    "robot": "tests/test_parity_gpu.py::test_step_matches_oracle_resynced",
    "task": "tests/test_parity_gpu.py::test_step_matches_oracle_resynced",
    "control": "tests/test_parity_gpu.py::test_step_matches_oracle_resynced",
    "episode_length": "tests/test_parity_gpu2.py::test_config5_pd_path_resynced_vs_oracle",
    "use_urdf_inertia": "tests/test_parity_gpu2.py::test_urdf_inertia_vs_oracle",
    "disable_termination": "tests/test_reference_pinned_gpu.py::test_step_kernel_pd_torque_matches_reference_pd_vectors",
    "precision": "tests/test_parity_gpu.py::test_fp64_engine_matches_oracle_tightly",
    "use_treadmill": "tests/test_parity_gpu2.py::test_treadmill_configs_basic_yaml_vs_oracle",
    "friction_model": "tests/test_parity_gpu3.py::test_friction_model_and_contact_erp_options_vs_oracle",
    "kp": "tests/test_reference_pinned_gpu.py::test_step_kernel_pd_torque_matches_reference_pd_vectors",
    "kd": "tests/test_reference_pinned_gpu.py::test_step_kernel_pd_torque_matches_reference_pd_vectors",
    "warmstart": "tests/test_parity_gpu2.py::test_fixed_sweep_variants_vs_oracle",
    "joint_limit": "tests/test_parity_gpu2.py::test_joint_limit_rows_vs_oracle",
    "solver_residual_threshold": "tests/test_parity_gpu2.py::test_residual_threshold_early_exit_vs_oracle",
    "contact_erp": "tests/test_parity_gpu3.py::test_friction_model_and_contact_erp_options_vs_oracle",
}


def case_id(case):
    f = case.field if isinstance(case.field, str) else "_".join(case.field)
    v = case.value if not isinstance(case.value, tuple) else "_".join(str(x) for x in case.value)
    return "%s_%s" % (f, ("%.4g" % v) if isinstance(v, float) else v)


def case_fields(case):
    return (case.field,) if isinstance(case.field, str) else tuple(case.field)


def scenario_config(scenario):
    """The scenario's configuration with every field of CASES at its default."""
    c = default_config(ROBOT_SOLO12, TASK_POINTGOAL if scenario in ("resynced_pointgoal", "reset") else TASK_WALK)
    c.num_history_stack = 1
    c.control = CONTROL_TORQUE
    if scenario == "resynced_limits":
        c.joint_limit = 0.3
    elif scenario == "resynced_lying":
        c.disable_termination = 1            # (a trunk on the ground is a fallen robot: baseEnv.py:169)
    elif scenario in ("treadmill_stance", "treadmill_stance_narrow"):
        c.use_treadmill = 1; c.control = CONTROL_PD
        if scenario == "treadmill_stance_narrow":
            # half width 0.5: all four feet on the strip; 0.2: the feet of one side only -- and a strip slippery enough for that to show
            c.treadmill_offset = 0.25; c.treadmill_friction = 0.1
    elif scenario == "reset":
        c.use_treadmill = 1; c.episode_length = 3
        c.num_history_stack = 0              # (the engine fills the history from the settle steps: settle_min >= num_history_stack)
    elif scenario == "history":
        c.episode_length = 7
    return c


def case_config(case, changed=True):
    c = scenario_config(case.scenario)
    if changed:
        values = case.value if isinstance(case.value, tuple) else (case.value,)
        for f, v in zip(case_fields(case), values):
            setattr(c, f, v)
    return c


def threads():
    try:
        return min(16, len(os.sched_getaffinity(0)))
    except AttributeError:
        return 4


class OracleSide:
    """The oracle behind the call shape the scenarios use (numpy in and out; actions arrive as float32, as they cross the engine's ABI)."""

    def __init__(self, cfg, N, seed):
        from oracle.oracle_py import Oracle
        self.o = Oracle(cfg, N, seed=seed, threads=threads())
        self.cfg, self.N = cfg, N

    def caps(self, contacts, limits):
        self.o.set_caps(contacts, limits)

    def reset(self):
        return self.o.reset()

    def step(self, a):
        obs, rew, done, _ = self.o.step(np.asarray(a, np.float32).astype(np.float64))
        return obs, rew, done != 0

    def get_state(self, i):
        return self.o.get_state(i)

    def set_state(self, i, s):
        self.o.set_state(i, s)


def obs_diff(a, b, D):
    """|a - b| with the euler entries compared modulo the wrap of the reference's (euler % 2)/2 (tests/test_parity_gpu.py::obs_diff)"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    for base in range(0, d.shape[-1], D):
        e = d[..., base + 1:base + 4]
        d[..., base + 1:base + 4] = np.minimum(e, np.abs(1.0 - e))
    return d


def _actions(scenario, rng, t, n):
    if scenario == "resynced_lying":
        return (0.05 * rng.uniform(-1, 1, size=(N_ENVS, n))).astype(np.float32)
    if scenario in ("treadmill_stance", "treadmill_stance_narrow"):
        return (0.02 * rng.uniform(-1, 1, size=(N_ENVS, n))).astype(np.float32)        # PD targets within +-0.2 rad of the stance
    if scenario == "history":
        return (0.3 * rng.uniform(-1, 1, size=(N_ENVS, n))).astype(np.float32)
    return (rng.uniform(-1.2, 1.2, size=(N_ENVS, n)) * (0.3 if t < N_STEPS // 2 else 1.0)).astype(np.float32)


def _dq(a, b, n):
    return float(np.abs(np.array(a.q)[:n] - np.array(b.q)[:n]).max())


def run_scenario(case, lead, follow, strip_side="follow"):
    """`lead` and `follow`: two sides (the engine and the oracle with the same configuration; or, for the condition on the inputs, the
    oracle with the changed value and the oracle with the default).  Before every step `follow` is loaded with `lead`'s state.
    Returns dict(samples = the compared quantity over the samples that count, mask_mismatch, total, extra) -- the caller applies its bounds.
    `strip_side`: whose contact mask selects the on-strip samples (the oracle running the changed value)."""
    sc, n = case.scenario, 12
    D = lead.cfg.state_dim
    if sc in ("resynced_limits", "resynced_lying"):
        for s in (lead, follow):
            s.caps(8, 4)                        # the oracle solves the rows the engine's slots hold (tests/test_parity_gpu2.py::test_joint_limit_rows_vs_oracle)
    rng = np.random.default_rng(0)
    out = dict(samples=[], mask_mismatch=0, total=0, extra={})
    ol, of = lead.reset(), follow.reset()
    if sc == "reset":
        return _reset_scenario(case, lead, follow, ol, of, rng, out)
    if sc == "history":
        out["extra"]["reset_obs"] = (ol, of)
    if sc == "resynced_lying":
        for i in range(N_ENVS):                  # upside down just above the ground, the legs spread at random, at rest
            s = lead.get_state(i)
            s.pos[2] = LYING_HEIGHT; s.quat[:] = [1.0, 0.0, 0.0, 0.0]
            for j in range(n):
                s.q[j] = float(rng.uniform(-1.0, 1.0)); s.qd[j] = 0.0
            s.lin_vel[:] = [0.0, 0.0, 0.0]; s.ang_vel[:] = [0.0, 0.0, 0.0]
            lead.set_state(i, s)
    limit_rows = strip = 0
    for t in range(N_STEPS):
        for i in range(N_ENVS):
            follow.set_state(i, lead.get_state(i))
        a = _actions(sc, rng, t, n)
        obs_l, rew_l, done_l = lead.step(a)
        obs_f, rew_f, done_f = follow.step(a)
        if sc == "history":
            # the whole observation, ended episodes (post-reset rows) included; a side with fewer levels reads as zeros beyond its own
            w = max(obs_l.shape[1], obs_f.shape[1])
            pl, pf = np.zeros((N_ENVS, w)), np.zeros((N_ENVS, w))
            pl[:, :obs_l.shape[1]] = obs_l; pf[:, :obs_f.shape[1]] = obs_f
            out["samples"] += list(obs_diff(pl, pf, D).max(axis=1))
            out["extra"].setdefault("done_equal", []).append(bool(np.array_equal(done_l, done_f)))
            out["extra"].setdefault("resets", []).append(int(done_l.sum()))
            out["total"] += N_ENVS
            continue
        for i in range(N_ENVS):
            if done_l[i] or done_f[i]:
                continue
            sl, sf = lead.get_state(i), follow.get_state(i)
            out["total"] += 1
            out["mask_mismatch"] += sl.contact_mask != sf.contact_mask
            limit_rows += bool((np.abs(np.array(sf.q)[:n]) >= lead.cfg.joint_limit).any())
            if case.quantity == "joint_angle_on_strip":
                if not ((sl if strip_side == "lead" else sf).contact_mask >> 24):
                    continue
                strip += 1
            out["samples"].append(abs(float(rew_l[i]) - float(rew_f[i])) if case.quantity == "reward" else _dq(sl, sf, n))
    out["extra"].update(limit_rows=limit_rows, strip=strip)
    return out


def _reset_scenario(case, lead, follow, ol, of, rng, out):
    """reset() and the auto-reset after episode_length = 3 steps: the state both sides reset to (tests/test_parity_gpu.py::test_reset_matches_oracle)"""
    n, D = 12, lead.cfg.state_dim
    obs_pairs = [(ol, of)]

    def collect():
        for i in range(N_ENVS):
            sl, sf = lead.get_state(i), follow.get_state(i)
            out["total"] += 1
            out["mask_mismatch"] += sl.contact_mask != sf.contact_mask
            out["samples"].append(abs(abs(sl.treadmill_y) - abs(sf.treadmill_y)) if case.quantity == "treadmill_y" else
                                  float(np.abs(np.array(sl.goal) - np.array(sf.goal)).max()) if case.quantity == "goal" else
                                  float(np.abs(state_vec(sl, n) - state_vec(sf, n)).max()))
            out["extra"].setdefault("rng_equal", []).append(sl.rng_counter == sf.rng_counter and sl.timestep == sf.timestep == 0)
            out["extra"].setdefault("side_equal", []).append(np.sign(sl.treadmill_y) == np.sign(sf.treadmill_y))
            out["extra"].setdefault("treadmill_y", []).append(sl.treadmill_y)

    collect()
    for t in range(3):
        for i in range(N_ENVS):
            follow.set_state(i, lead.get_state(i))
        a = (0.1 * rng.uniform(-1, 1, size=(N_ENVS, n))).astype(np.float32)
        obs_l, _, done_l = lead.step(a)
        obs_f, _, done_f = follow.step(a)
    out["extra"]["timeouts"] = (int(done_l.sum()), int(done_f.sum()))
    obs_pairs.append((obs_l, obs_f))
    collect()                                         # every env has just timed out and been reset by the step itself
    out["extra"]["obs_max"] = [float(obs_diff(x, y, D).max()) for x, y in obs_pairs]
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_case_moves_the_oracle(case):
    """Changed value vs default on the oracle alone, from identical states: median of the compared quantity >= 1e-3 over the samples the
    GPU test asserts on (measured medians: the table in DESIGN.md section 4, "Config fields and their tests")."""
    lead = OracleSide(case_config(case, True), N_ENVS, seed=3)
    follow = OracleSide(case_config(case, False), N_ENVS, seed=3)
    r = run_scenario(case, lead, follow, strip_side="lead")
    s = np.asarray(r["samples"])
    print("config_field/%s: oracle alone, changed vs default: n %d of %d  median %.3e  p10 %.3e  extra %s" % (
        case_id(case), s.size, r["total"], np.median(s), np.percentile(s, 10), {k: v for k, v in r["extra"].items() if np.isscalar(v)}))
    assert np.median(s) >= 1e-3, np.median(s)
    if case.quantity == "joint_angle_on_strip":
        assert s.size > 0.5 * r["total"], (s.size, r["total"])          # more than half of the samples qualify
    else:
        assert s.size > 0.5 * N_ENVS * N_STEPS or case.scenario == "reset"
    if case.scenario == "resynced_limits":
        assert r["extra"]["limit_rows"] > 0.5 * r["total"]              # limit rows exist in most samples


def test_every_config_field_is_exercised():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    in_cases = {f for c in CASES for f in case_fields(c)}
    names = [n for n, _ in SoloConfig._fields_]
    assert not in_cases & set(COVERED_ELSEWHERE), in_cases & set(COVERED_ELSEWHERE)
    missing = [n for n in names if n not in in_cases and n not in COVERED_ELSEWHERE]
    assert not missing, "solorl_config fields no test moves off their defaults: %s" % missing
    assert set(COVERED_ELSEWHERE) | in_cases == set(names), (set(COVERED_ELSEWHERE) | in_cases) - set(names)
    for field, where in COVERED_ELSEWHERE.items():
        path, func = where.split("::")
        assert os.path.exists(os.path.join(root, path)), where
        mod = importlib.import_module(path[:-3].replace("/", "."))
        assert hasattr(mod, func), where
        assert field in inspect.getsource(getattr(mod, func)), "%s does not mention %r" % (where, field)
