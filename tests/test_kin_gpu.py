"""solorl_kinematics on the GPU (include/solorl.h; solorl_amd/kinematics.py, SoloVecEnv.get_kinematics).

The kernel's rows against the rows of the stand-alone host program (tests/host/rows_main.cpp: the same per-env function compiled by
g++) to |err| <= 1e-10 max(1, |value|), and through the three comparisons of tests/test_kin_host.py on the device's own rows (oracle
prim_points, oracle energy_momentum, numpy forward kinematics and its central differences) -- for both robots and both inertia rules,
n = 1, 5, one more than the kernel's envs per workgroup, and 67 (four workgroups, the last one ragged).  Then the call's contract:
masked rows keep every byte, bad arguments are refused by name, a captured call follows the states it is replayed on,
SoloVecEnv.get_kinematics is the same call, prim_force is lambda_prev / sim_dt under the contact mask bit for bit.
Two physics checks on the engine itself, bounded by the ORACLE's own deviation on the same input (tests/golden/kin_measured.json,
written by tests/golden/make_golden_kin.py on the CPU): linear momentum in free flight, and the summed normal force of a PD stance."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from solorl_amd import _native
from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK, PRECISION_F64
from solorl_amd.kinematics import kinematics, KinBatch, ENVS_PER_WORKGROUP, ROW_WORDS, FOOT_PRIMS
from solorl_amd.state import StateBatch
from tests import kin_util as ku
from tests.golden import make_golden_kin as gk

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 5, ENVS_PER_WORKGROUP + 1, max(ENVS_PER_WORKGROUP + 1, 67))
MEASURED = json.load(open(os.path.join(ku.ROOT, "tests", "golden", "kin_measured.json")))

_HOST_ROWS = {}


def _case(robot, urdf):
    """(cfg, the 64 seeded states + the first three again = 67, the host program's rows for them), once per process"""
    if (robot, urdf) not in _HOST_ROWS:
        cfg, states = ku.inputs(robot, urdf)
        states = states + states[:3]
        _HOST_ROWS[(robot, urdf)] = (cfg, states, ku.run_kin_main(cfg, states))
    return _HOST_ROWS[(robot, urdf)]


def _device_rows(cfg, states, **kw):
    return kinematics(cfg, StateBatch.from_env_states(states, DEV), **kw).data.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("robot,urdf", ku.CASES)
def test_kernel_rows_equal_the_host_program(robot, urdf, n):
    cfg, states, host = _case(robot, urdf)
    rows = _device_rows(cfg, states[:n])
    bad = ~ku.close(rows, host[:n], ku.TOL)
    assert not bad.any(), (np.argwhere(bad)[:5], np.abs(rows - host[:n]).max())
    if n == SIZES[-1]:
        ku.check_rows(robot, cfg, states[:n], rows)            # the three comparisons on the device's own rows


def test_masked_rows_keep_every_byte():
    cfg, states, _ = _case(1, 0)
    n = len(states)
    sb = StateBatch.from_env_states(states, DEV)
    full = kinematics(cfg, sb)
    mask = (torch.arange(n, device=DEV) % 3 != 1)
    mask[ENVS_PER_WORKGROUP:2 * ENVS_PER_WORKGROUP] = False          # a workgroup with nothing to do
    for m in (mask, mask.to(torch.uint8) * 7):
        out = KinBatch(data=torch.full((n, ROW_WORDS), float("nan"), dtype=torch.float64, device=DEV))
        out.bytes().fill_(0xA5)
        # a masked row is not read either: poison them in the input
        poisoned = sb.clone()
        poisoned.data[~mask] = float("nan")
        got = kinematics(cfg, poisoned, mask=m, out=out)
        assert got is out
        b, sel = out.bytes().cpu().numpy(), mask.cpu().numpy()
        assert (b[~sel] == 0xA5).all()
        assert (b[sel] == full.bytes().cpu().numpy()[sel]).all()


def test_bad_arguments_are_refused_by_name():
    L = _native.lib()
    cfg, states, _ = _case(1, 0)
    sb = StateBatch.from_env_states(states[:4], DEV)
    out = KinBatch(4, DEV)
    before = out.data.clone()
    ps, po = C.c_void_p(sb.data.data_ptr()), C.c_void_p(out.data.data_ptr())
    bad_robot = cfg.copy(); bad_robot.robot = -1
    bad_dt = cfg.copy(); bad_dt.sim_dt = 0.0
    for c, s, o, n in ((None, ps, po, 4), (C.byref(cfg), None, po, 4), (C.byref(cfg), ps, None, 4), (C.byref(cfg), ps, po, 0),
                       (C.byref(bad_robot), ps, po, 4), (C.byref(bad_dt), ps, po, 4)):
        assert L.solorl_kinematics(c, s, None, n, o, 0, None) == -1
        assert L.solorl_last_error().startswith(b"solorl_kinematics:")
    torch.cuda.synchronize()
    assert torch.equal(out.data, before)                   # nothing was launched
    with pytest.raises(_native.SoloRLError):
        kinematics(cfg, StateBatch(4, "cpu"))              # no CPU fallback


def test_captured_call_follows_the_states():
    cfg, states, _ = _case(1, 1)
    a = StateBatch.from_env_states(states[:20], DEV)
    b = StateBatch.from_env_states(states[20:40], DEV)
    want_a, want_b = kinematics(cfg, a).data.clone(), kinematics(cfg, b).data.clone()
    sb, out = a.clone(), KinBatch(20, DEV)
    kinematics(cfg, sb, out=out)                           # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        kinematics(cfg, sb, out=out)
    out.data.zero_()
    g.replay()
    assert torch.equal(out.data, want_a)
    sb.data.copy_(b.data)
    g.replay()
    assert torch.equal(out.data, want_b)
    assert not torch.equal(want_a, want_b)


@pytest.mark.parametrize("handle", ["fp32", "fp64", "lane"])
def test_get_kinematics_is_the_same_call_and_forces_are_the_cached_impulses(handle, monkeypatch):
    from solorl_amd.vec_env import SoloVecEnv
    monkeypatch.delenv("SOLORL_TEAM", raising=False)
    monkeypatch.delenv("SOLORL_SORT", raising=False)
    if handle == "lane":
        monkeypatch.setenv("SOLORL_TEAM", "0")
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    if handle == "fp64":
        cfg.precision = PRECISION_F64
    env = SoloVecEnv(cfg, 8, device=DEV, seed=3)
    env.reset()
    g = torch.Generator(device=DEV); g.manual_seed(17)
    for _ in range(20):
        env.step_inplace((torch.rand(8, 12, device=DEV, generator=g) * 2 - 1).contiguous())
    sb = env.get_states()
    want = kinematics(env.cfg, sb)
    got = env.get_kinematics()
    assert torch.equal(got.bytes(), want.bytes())
    assert torch.equal(env.get_kinematics(states=sb).bytes(), want.bytes())
    # masked: the selected rows only
    mask = torch.arange(8, device=DEV) % 2 == 0
    part = env.get_kinematics(mask=mask)
    assert torch.equal(part.bytes()[mask], want.bytes()[mask]) and not part.data[~mask].any()
    # normal forces = the cached impulses of the last sub-step over sim_dt, where the primitive touched
    bits = ((sb.contact_mask.unsqueeze(1) >> torch.arange(24, device=DEV, dtype=torch.int32)) & 1).bool()
    ref = torch.where(bits, sb.lambda_prev / cfg.sim_dt, torch.zeros_like(sb.lambda_prev))
    assert torch.equal(want.prim_force.contiguous().view(torch.int64), ref.contiguous().view(torch.int64))
    assert bits.any() and (want.prim_force > 0).any()                      # robots on the ground after 20 steps
    assert torch.equal(want.foot_force, want.prim_force[:, list(FOOT_PRIMS)]) and torch.equal(want.foot_pos, want.prim_point[:, list(FOOT_PRIMS)])
    env.close()


def test_free_flight_momentum_within_the_oracles_own_deviation():
    """fp64 handle, damping 0, the base 1 m up, seeded joint rates, zero torque, 10 steps: lin_mom xy stays, z falls by M g t.  Allowed:
    10 x the oracle's own deviation on the same input (tests/golden/kin_measured.json)."""
    from solorl_amd.vec_env import SoloVecEnv
    cfg = gk.free_flight_cfg()
    env = SoloVecEnv(cfg, 1, device=DEV, seed=1)
    env.reset()
    s = gk.free_flight_state(env.get_states().env_state(0))
    env.set_states(StateBatch.from_env_states([s], DEV))
    zero = torch.zeros(1, 12, device=DEV)
    p = [env.get_kinematics().lin_mom[0].clone()]
    for _ in range(gk.FREE_STEPS):
        env.step_inplace(zero)
        p.append(env.get_kinematics().lin_mom[0].clone())
    assert int(env.get_states().contact_mask[0]) & 0xFFFFFF == 0
    kin = env.get_kinematics()
    assert abs(float(kin.mass[0]) - gk.total_mass()) < 1e-12
    xy, z = gk.momentum_deviation(torch.stack(p).cpu().numpy(), gk.total_mass(), cfg.gravity, cfg.frame_skip * cfg.sim_dt)
    ref = MEASURED["free_flight"]
    print("free flight: momentum deviation xy %.3e z %.3e kg m/s (oracle %.3e, %.3e)" % (xy, z, ref["xy"], ref["z"]))
    assert ref["steps"] == gk.FREE_STEPS
    assert xy <= 10 * ref["xy"] and z <= 10 * ref["z"]
    env.close()


def test_stance_normal_forces_within_the_oracles_own_figure():
    """fp64 handle, tests/golden/stand_pd_start.json, the fixture's PD gains and actions, 200 steps: |sum prim_force - M g| / (M g), mean
    over the steps, at most 3 x the oracle's own figure for sum last_lambda / sim_dt on the same run."""
    from solorl_amd.vec_env import SoloVecEnv
    from tests.golden.make_golden import stand_cfg, stand_action
    from tests.util import load_state
    cfg = stand_cfg(); cfg.precision = PRECISION_F64
    env = SoloVecEnv(cfg, 1, device=DEV, seed=1)
    env.reset()
    env.set_state(0, load_state("stand_pd_start.json"))
    mg = gk.total_mass() * cfg.gravity
    f = []
    for t in range(gk.STANCE_STEPS):
        env.step_inplace(torch.from_numpy(stand_action(t)[None]).to(DEV, torch.float32).contiguous())
        f.append(env.get_kinematics().prim_force.sum().clone())
    rel = (torch.stack(f) - mg).abs() / mg
    ref = MEASURED["stance"]
    print("stance: |sum F - M g| / (M g) mean %.4f max %.4f (oracle mean %.4f max %.4f)" % (float(rel.mean()), float(rel.max()), ref["mean_rel"], ref["max_rel"]))
    assert ref["steps"] == gk.STANCE_STEPS
    assert float(rel.mean()) <= 3 * ref["mean_rel"]
    assert (torch.stack(f) > 0).all()                      # it stands on something at every step
    env.close()
