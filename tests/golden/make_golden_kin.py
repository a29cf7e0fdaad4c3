#!/usr/bin/env python3
"""Writes tests/golden/kin_measured.json: the fp64 oracle's OWN deviations on the two physics checks of tests/test_kin_gpu.py, which
bound the engine's (nothing in the file is taken from the engine; runs on the CPU).

  free_flight   Solo12, damping 0, the base 1 m up, seeded joint angles and rates, zero torque, 10 control steps.  Linear momentum
                from oracle_energy_momentum after every step: "xy" = max |p_xy(t) - p_xy(0)|, "z" = max |p_z(t) - (p_z(0) - M g t)|
                [kg m/s].  Not rounding: the integrator holds the joint RATES over a sub-step while the configuration moves, so the
                momentum of the same generalised velocities drifts at O(dt).
  stance        Solo12 from tests/golden/stand_pd_start.json, the fixture's PD gains and actions (make_golden.stand_cfg / stand_action),
                200 control steps.  F(t) = sum over primitives of oracle_last_lambda / sim_dt after step t; "mean_rel" = the mean over
                the 200 steps of |F - M g| / (M g), "max_rel" its maximum (recorded, not used as a bound).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

FREE_STEPS, STANCE_STEPS = 10, 200


def free_flight_cfg():
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK, PRECISION_F64
    c = default_config(ROBOT_SOLO12, TASK_WALK)
    c.damping = 0.0; c.disable_termination = 1; c.precision = PRECISION_F64
    return c


def free_flight_state(s):
    """the start of the free-flight check written into EnvState s (a state after reset): 1 m up, seeded pose and rates"""
    rng = np.random.default_rng(77)
    s.pos[:] = [0.0, 0.0, 1.0]
    q = rng.normal(size=4); q /= np.linalg.norm(q); s.quat[:] = list(q)
    s.lin_vel[:] = list(rng.uniform(-0.5, 0.5, 3)); s.ang_vel[:] = list(rng.uniform(-1, 1, 3))
    for j in range(12):
        s.q[j] = rng.uniform(-1, 1); s.qd[j] = rng.uniform(-5, 5); s.tau[j] = 0.0
    for p in range(24):
        s.lambda_prev[p] = 0.0
    s.contact_mask = 0
    return s


def momentum_deviation(p, mass, g, dt_step):
    """p [T + 1, 3]: linear momentum at the start and after each step -> (xy, z) deviations from constant / falling by M g t"""
    p = np.asarray(p)
    t = np.arange(len(p)) * dt_step
    return float(np.abs(p[:, :2] - p[0, :2]).max()), float(np.abs(p[:, 2] - (p[0, 2] - mass * g * t)).max())


def total_mass(robot_json="solo12.json"):
    return sum(l["mass"] for l in json.load(open(os.path.join(ROOT, "solorl_amd", "models", robot_json)))["links"])


def measure_free_flight():
    from oracle.oracle_py import Oracle
    c = free_flight_cfg()
    o = Oracle(c, 1, seed=1)
    o.reset()
    o.set_state(0, free_flight_state(o.get_state(0)))
    p = [o.energy_momentum(0)["p"]]
    for t in range(FREE_STEPS):
        o.step(np.zeros((1, 12)))
        assert o.get_state(0).contact_mask & 0xFFFFFF == 0
        p.append(o.energy_momentum(0)["p"])
    xy, z = momentum_deviation(p, total_mass(), c.gravity, c.frame_skip * c.sim_dt)
    return dict(xy=xy, z=z, steps=FREE_STEPS)


def measure_stance():
    from oracle.oracle_py import Oracle
    from tests.golden.make_golden import stand_cfg, stand_action, state_from_dict
    c = stand_cfg()
    o = Oracle(c, 1, seed=1)
    o.reset()
    o.set_state(0, state_from_dict(json.load(open(os.path.join(HERE, "stand_pd_start.json")))))
    mg = total_mass() * c.gravity
    rel = []
    for t in range(STANCE_STEPS):
        o.step(stand_action(t)[None])
        rel.append(abs(o.last_lambda(0).sum() / c.sim_dt - mg) / mg)
    return dict(mean_rel=float(np.mean(rel)), max_rel=float(np.max(rel)), steps=STANCE_STEPS)


if __name__ == "__main__":
    out = dict(free_flight=measure_free_flight(), stance=measure_stance())
    json.dump(out, open(os.path.join(HERE, "kin_measured.json"), "w"), indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))
