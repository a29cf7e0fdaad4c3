"""solorl_dynamics on the GPU (include/solorl.h; solorl_amd/dyn_tensors.py, SoloVecEnv.get_dynamics).

The kernel's rows against the rows of the stand-alone host program (tests/host/rows_main.cpp: the same per-env function compiled by
g++) to |err| <= 1e-10 max(1, |value|), the mass matrix to 1e-10 sqrt(M_aa M_bb), and through the five comparisons of
tests/dyn_util.py check_rows on the device's own rows (the oracle's mass matrix, bias and forward dynamics, the device's own
solorl_kinematics rows, the numpy restatement of the foot Jacobians) -- for both robots and both inertia rules, n = 1, 5, one more than
the kernel's envs per workgroup, and three workgroups plus five rows.  Then the call's contract: masked rows keep every byte, bad
arguments are refused by name, a captured call follows the states it is replayed on, SoloVecEnv.get_dynamics is the same call.
Last, the engine against its own tensors: the acceleration of one free-flight sub-step is solve(M, tau - bias).  Measured on an
MI355X (fp64 handle, 8 envs, max over envs and coordinates, in rad/s^2 resp. m/s^2 beside max |B| = 1750 / 983):
  Solo12: |C - B| 5.2e-12, |A - B| 5.6e-12, |A - C| 3.6e-12;   Solo8: |C - B| 3.3e-12, |A - B| 2.3e-12, |A - C| 3.3e-12."""
import ctypes as C

import numpy as np
import pytest
import torch

from solorl_amd import _native
from solorl_amd.config import default_config, ROBOT_SOLO8, ROBOT_SOLO12, TASK_WALK, PRECISION_F64, CONTROL_TORQUE
from solorl_amd.dyn_tensors import dynamics, velocity, DynBatch, ENVS_PER_WORKGROUP, ROW_WORDS
from solorl_amd.kinematics import kinematics
from solorl_amd.state import StateBatch
from tests import dyn_util as du
from tests import kin_util as ku
from tests.util import clone

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 5, ENVS_PER_WORKGROUP + 1, 3 * ENVS_PER_WORKGROUP + 5)      # the last: four workgroups, the last one ragged

_HOST_ROWS = {}


def _case(robot, urdf):
    """(cfg, the first SIZES[-1] of the 64 seeded states taken alternately from the random and the rollout half, the host program's
    rows for them), once per process"""
    if (robot, urdf) not in _HOST_ROWS:
        cfg, states = ku.inputs(robot, urdf)
        states = [states[(i % 2) * 32 + i // 2] for i in range(64)][:SIZES[-1]]
        _HOST_ROWS[(robot, urdf)] = (cfg, states, du.run_dyn_main(cfg, states))
    return _HOST_ROWS[(robot, urdf)]


def _device_rows(cfg, states, **kw):
    return dynamics(cfg, StateBatch.from_env_states(states, DEV), **kw).data.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("robot,urdf", ku.CASES)
def test_kernel_rows_equal_the_host_program(robot, urdf, n):
    cfg, states, host = _case(robot, urdf)
    assert SIZES[-1] <= 64 and len(states) == SIZES[-1]
    rows = _device_rows(cfg, states[:n])
    bad = ~ku.close(rows, host[:n], ku.TOL)
    assert not bad.any(), (np.argwhere(bad)[:5], np.abs(rows - host[:n]).max())
    M, Mh = du.member(rows, "mass_matrix"), du.member(host[:n], "mass_matrix")
    for i in range(n):
        assert du.scaled_m_close(M[i], Mh[i]).all(), (i, np.abs(M[i] - Mh[i]).max())
    if n == SIZES[-1]:
        # the five comparisons on the device's own rows, with the device's own kinematics rows; bias again without damping
        kin = kinematics(cfg, StateBatch.from_env_states(states, DEV)).data.cpu().numpy()
        du.check_rows(robot, cfg, states, rows, kin)
        cfg0 = du.no_damping(cfg)
        du.check_rows(robot, cfg0, states, _device_rows(cfg0, states), kin, restatement=False)


def test_masked_rows_keep_every_byte():
    cfg, states, _ = _case(1, 0)
    n = len(states)
    sb = StateBatch.from_env_states(states, DEV)
    full = dynamics(cfg, sb)
    mask = (torch.arange(n, device=DEV) % 3 != 1)
    mask[ENVS_PER_WORKGROUP:2 * ENVS_PER_WORKGROUP] = False          # a workgroup with nothing to do
    for m in (mask, mask.to(torch.uint8) * 7):
        out = DynBatch(data=torch.full((n, ROW_WORDS), float("nan"), dtype=torch.float64, device=DEV))
        out.bytes().fill_(0xA5)
        # a masked row is not read either: poison them in the input
        poisoned = sb.clone()
        poisoned.data[~mask] = float("nan")
        got = dynamics(cfg, poisoned, mask=m, out=out)
        assert got is out
        b, sel = out.bytes().cpu().numpy(), mask.cpu().numpy()
        assert (b[~sel] == 0xA5).all()
        assert (b[sel] == full.bytes().cpu().numpy()[sel]).all()


def test_bad_arguments_are_refused_by_name():
    L = _native.lib()
    cfg, states, _ = _case(1, 0)
    sb = StateBatch.from_env_states(states[:4], DEV)
    out = DynBatch(4, DEV)
    out.data.fill_(3.0)
    before = out.data.clone()
    ps, po = C.c_void_p(sb.data.data_ptr()), C.c_void_p(out.data.data_ptr())
    bad_robot = cfg.copy(); bad_robot.robot = -1
    bad_g = cfg.copy(); bad_g.gravity = float("nan")
    nan_k = cfg.copy(); nan_k.damping = float("inf")
    neg_k = cfg.copy(); neg_k.damping = -1.0
    for c, s, o, n in ((None, ps, po, 4), (C.byref(cfg), None, po, 4), (C.byref(cfg), ps, None, 4), (C.byref(cfg), ps, po, 0),
                       (C.byref(bad_robot), ps, po, 4), (C.byref(bad_g), ps, po, 4), (C.byref(nan_k), ps, po, 4), (C.byref(neg_k), ps, po, 4)):
        assert L.solorl_dynamics(c, s, None, n, o, 0, None) == -1
        assert L.solorl_last_error().startswith(b"solorl_dynamics:")
    torch.cuda.synchronize()
    assert torch.equal(out.data, before)                   # nothing was launched
    with pytest.raises(_native.SoloRLError):
        dynamics(cfg, StateBatch(4, "cpu"))                # no CPU fallback


def test_captured_call_follows_the_states():
    cfg, states, _ = _case(1, 1)
    a = StateBatch.from_env_states(states[:20], DEV)
    b = StateBatch.from_env_states(states[20:40], DEV)
    want_a, want_b = dynamics(cfg, a).data.clone(), dynamics(cfg, b).data.clone()
    sb, out = a.clone(), DynBatch(20, DEV)
    dynamics(cfg, sb, out=out)                             # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dynamics(cfg, sb, out=out)
    out.data.zero_()
    g.replay()
    assert torch.equal(out.data, want_a)
    sb.data.copy_(b.data)
    g.replay()
    assert torch.equal(out.data, want_b)
    assert not torch.equal(want_a, want_b)


@pytest.mark.parametrize("handle", ["fp32", "fp64", "lane"])
def test_get_dynamics_is_the_same_call(handle, monkeypatch):
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
    want = dynamics(env.cfg, sb)
    got = env.get_dynamics()
    assert torch.equal(got.bytes(), want.bytes())
    assert torch.equal(env.get_dynamics(states=sb).bytes(), want.bytes())
    assert torch.isfinite(want.data).all() and (want.mass_matrix.diagonal(dim1=1, dim2=2) > 0).all()
    # masked: the selected rows only
    mask = torch.arange(8, device=DEV) % 2 == 0
    part = env.get_dynamics(mask=mask)
    assert torch.equal(part.bytes()[mask], want.bytes()[mask]) and not part.data[~mask].any()
    # the generalised velocity the tensors are written for
    v = velocity(sb)
    assert v.shape == (8, 18) and torch.equal(v[:, 0:3], sb.lin_vel) and torch.equal(v[:, 3:6], sb.ang_vel) and torch.equal(v[:, 6:], sb.qd)
    env.close()


@pytest.mark.parametrize("robot", (ROBOT_SOLO12, ROBOT_SOLO8))
def test_the_engine_obeys_its_own_tensors(robot):
    """fp64 handle, one sub-step per step, torque control, 8 envs 3 m up with a tenth of the seeded rates, actions in +-0.1.
    A = (v' - v) / sim_dt of one step, B = the oracle's forward dynamics of the same states, C = solve(M, tau - bias) from the device
    rows:  |C - B| <= 1e-6 max|B|  and  |A - C| <= 10 max(|A - B|, 1e-12 max|B|)."""
    from oracle.oracle_py import Oracle
    from solorl_amd.vec_env import SoloVecEnv
    N = 8
    cfg = default_config(robot, TASK_WALK)
    cfg.precision = PRECISION_F64; cfg.frame_skip = 1; cfg.control = CONTROL_TORQUE; cfg.disable_termination = 1
    assert cfg.damping == 0.04
    nq, nv = cfg.n_joints, 6 + cfg.n_joints
    env = SoloVecEnv(cfg, N, device=DEV, seed=5)
    env.reset()
    rng = np.random.default_rng(4242 + robot)
    seeded = ku.random_states(cfg, N, rng)
    start = []
    for i, r in enumerate(seeded):
        s = env.get_states().env_state(i)                  # a state after reset: task members and counters as the engine made them
        s.pos[:] = [r.pos[0], r.pos[1], 3.0]; s.quat[:] = list(r.quat)
        s.lin_vel[:] = [0.1 * x for x in r.lin_vel]; s.ang_vel[:] = [0.1 * x for x in r.ang_vel]
        for j in range(12):
            s.q[j] = r.q[j] if j < nq else 0.0
            s.qd[j] = 0.1 * r.qd[j] if j < nq else 0.0
            s.tau[j] = 0.0
        for p in range(24):
            s.lambda_prev[p] = 0.0
        s.contact_mask = 0
        start.append(s)
    env.set_states(StateBatch.from_env_states(start, DEV))
    act = torch.from_numpy(rng.uniform(-0.1, 0.1, (N, nq)).astype(np.float32)).to(DEV).contiguous()
    before = env.get_states().clone()
    dyn = env.get_dynamics().clone()
    env.step_inplace(act)
    after = env.get_states()
    assert not (after.contact_mask & 0xFFFFFF).any()
    v0, v1 = velocity(before).cpu().numpy()[:, :nv], velocity(after).cpu().numpy()[:, :nv]
    assert (np.abs(v1) < 0.9 * cfg.max_velocity).all()
    A = (v1 - v0) / cfg.sim_dt
    tau = act.cpu().numpy().astype(np.float64) * cfg.max_torque
    M, bias = dyn.mass_matrix.cpu().numpy()[:, :nv, :nv], dyn.bias.cpu().numpy()[:, :nv]
    orc = Oracle(cfg, 1)
    B, Cc = np.zeros((N, nv)), np.zeros((N, nv))
    for i in range(N):
        s = clone(before.env_state(i))
        for j in range(nq):
            s.tau[j] = tau[i, j]
        orc.set_state(0, s)
        B[i] = orc.forward_dynamics(0)[du.PERM[:nv]]
        Cc[i] = np.linalg.solve(M[i], np.concatenate((np.zeros(6), tau[i])) - bias[i])
    scale = np.abs(B).max()
    cb, ab, ac = np.abs(Cc - B).max(), np.abs(A - B).max(), np.abs(A - Cc).max()
    print("robot %d: max|B| %.3e  |C - B| %.3e  |A - B| %.3e  |A - C| %.3e (relative to max|B|: %.2e %.2e %.2e)"
          % (robot, scale, cb, ab, ac, cb / scale, ab / scale, ac / scale))
    assert cb <= 1e-6 * scale
    assert ac <= 10 * max(ab, 1e-12 * scale)
    env.close()
