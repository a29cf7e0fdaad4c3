"""The helper wavefront's base pose and next-R0 (duo_kernel_team, DESIGN section 4 "Helper wavefront": barrier D behind the sweep, the
leader's pose integration and the next sub-step's R0 on the helper while the main wavefront integrates the joints, barrier Z in front of
the epilogue) against the classic one-wavefront kernel (SOLORL_HELPER_WAVE=0), bitwise.  Same seed, same actions: observations, rewards,
done flags, the info arrays, the applied torques, the episode accumulators and every env's state (get_states) must be the same bits.

The shapes are the smallest at which this change can go wrong: frame_skip 1 (barrier Z directly behind the first sub-step, R0 never the
helper's) and 3 (an odd count) with N = 5 (a full workgroup, a ragged one, and empty ones in the padded grid that leave before any
barrier); N = 1; one, two and three history levels (the observation's deltas of the pose the helper integrated); pointgoal under PD
control; Solo8 on the treadmill; lying and free-falling envs under the LDS poison hook (anything read across D, A or Z before it is
written); a replayed graph.  Every Solo12 walk case asserts that its window holds a reset, counted on the classic kernel's done flags
(episodes of 25 steps in windows of 40: the time limit alone gives one) -- but for the two poison cases: the lying pose needs
disable_termination, which switches the time limit off as well, so their windows hold no reset by construction."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_WORD = "0x7fc00000"
INFO = ("timeout", "success", "nan_reset", "episode_length", "episode_reward", "goals_reached",
        "dr_stand", "dr_joint_pose", "dr_torque", "dr_balance", "dr_progress")
AIR, LYING = (0, 4), (1, 5)             # as tests/test_helper_base_gpu.py: one of each kind in either workgroup of N = 6
LYING_Z = (0.020, 0.025)


def _walk12(frame_skip=None, history=1, no_termination=False):
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    c = default_config(ROBOT_SOLO12, TASK_WALK); c.num_history_stack = history; c.episode_length = 25
    if frame_skip is not None:
        c.frame_skip = frame_skip
    if no_termination:                   # (a base below 0.05 m ends the episode: the lying envs would be reset by their first step)
        c.disable_termination = 1
    return c


def _named(name):
    from solorl_amd.config import config_from_dict, load_yaml, TASK_WALK, TASK_POINTGOAL, CONTROL_PD
    if name == "walk8_treadmill":
        c = config_from_dict(load_yaml(os.path.join(ROOT, "configs", "basic.yaml"))); c.task = TASK_WALK; c.episode_length = 30
        assert c.use_treadmill
    elif name == "pointgoal12_pd":
        c = config_from_dict(load_yaml(os.path.join(ROOT, "configs", "basic12.yaml"))); c.task = TASK_POINTGOAL; c.control = CONTROL_PD
        c.episode_length = 30
    else:
        raise KeyError(name)
    return c


def _env(monkeypatch, cfg, N, helper, seed=7, poison=None):
    from solorl_amd.vec_env import SoloVecEnv
    monkeypatch.setenv("SOLORL_HELPER_WAVE", str(helper))
    if poison is not None:
        monkeypatch.setenv("SOLORL_POISON_LDS", poison)
    env = SoloVecEnv(cfg, N, device=torch.device("cuda:0"), seed=seed, applied_torque=True)
    monkeypatch.delenv("SOLORL_HELPER_WAVE")
    if poison is not None:
        monkeypatch.delenv("SOLORL_POISON_LDS")
    assert env.get_property("helper_wave") == helper
    return env


def _place(a, b, air=(), lying=()):
    """after the reset: the `air` envs lifted to base z = 1.0 at rest, the `lying` envs laid on the ground with folded legs (the pose
    of tests/test_helper_base_gpu.py); both handles get the same rows"""
    s = a.get_states()
    assert torch.equal(s.bytes(), b.get_states().bytes())
    ql = float(a.cfg.joint_limit)
    for i in tuple(air) + tuple(lying):
        s.lin_vel[i] = 0; s.ang_vel[i] = 0; s.qd[i] = 0
    for i in air:
        s.pos[i, 2] = 1.0
    for k, i in enumerate(lying):
        s.pos[i, 2] = LYING_Z[k % len(LYING_Z)]
        s.quat[i] = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)
        s.q[i, :12] = torch.tensor([0.0, ql, -ql] * 4, dtype=torch.float64)
        s.lambda_prev[i] = 0
    a.set_states(s); b.set_states(s)


def _contacts(env):
    m = env.get_states().contact_mask.cpu()
    return [bin(int(v) & 0xFFFFFF).count("1") for v in m]


def _same_rollout(a, b, steps, seed=11, air=(), lying=()):
    """the same seeded U(-1, 1) actions on both handles: every per-step output of every step, then the accumulators and every env's
    state -> (resets counted on b's done flags, contacts per env after the first step)"""
    N, A = a.nenvs, a.act_dim
    assert torch.equal(a.reset(), b.reset())
    if air or lying:
        _place(a, b, air, lying)
    g = torch.Generator(device="cuda:0"); g.manual_seed(seed)
    resets, first = 0, None
    for k in range(steps):
        act = torch.rand(N, A, device="cuda:0", generator=g) * 2 - 1
        oa, ra, da, ia = a.step_inplace(act)
        ob, rb, db, ib = b.step_inplace(act)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
        assert torch.equal(a._tau, b._tau), k
        for f in INFO:
            assert torch.equal(ia[f], ib[f]), (k, f)
        resets += int(db.sum())
        if k == 0:
            first = _contacts(a)
            assert first == _contacts(b)
    torch.cuda.synchronize()
    assert torch.equal(a._ep_stats, b._ep_stats)
    assert torch.equal(a.get_states().bytes(), b.get_states().bytes())
    return resets, first


@pytest.mark.parametrize("frame_skip", [1, 3])
def test_substep_counts(gpu_device, monkeypatch, frame_skip):
    """4 x frame_skip + 1 barriers per step and role.  frame_skip 1: Z directly follows the first sub-step's D, and the only R0 is the
    main wavefront's own; 3: an odd count, the helper's R0 twice.  N = 5: a full workgroup, a ragged one, empty ones in the grid"""
    on, off = _env(monkeypatch, _walk12(frame_skip), 5, 1), _env(monkeypatch, _walk12(frame_skip), 5, 0)
    resets, _ = _same_rollout(on, off, 40)
    assert resets > 0
    on.close(); off.close()


def test_one_env(gpu_device, monkeypatch):
    """three idle teams beside the one env: their helper lanes integrate no base"""
    on, off = _env(monkeypatch, _walk12(), 1, 1), _env(monkeypatch, _walk12(), 1, 0)
    resets, _ = _same_rollout(on, off, 40)
    assert resets > 0
    on.close(); off.close()


@pytest.mark.parametrize("history", [1, 2, 3])
def test_history_levels(gpu_device, monkeypatch, history):
    """L.H = 1, 2, 3: every level of the observation's deltas is taken against the pose the helper integrated (the history push itself
    stays on the main wavefront)"""
    on, off = _env(monkeypatch, _walk12(history=history), 5, 1), _env(monkeypatch, _walk12(history=history), 5, 0)
    resets, _ = _same_rollout(on, off, 40)
    assert resets > 0
    on.close(); off.close()


@pytest.mark.parametrize("name,N,steps", [("pointgoal12_pd", 9, 60),       # limit rows, quiet teams; the goal patch at a reset
                                          ("walk8_treadmill", 5, 60)])     # Solo8: HK and the lane map of the other robot; C.tmy
def test_other_tasks_and_robot(gpu_device, monkeypatch, name, N, steps):
    on, off = _env(monkeypatch, _named(name), N, 1), _env(monkeypatch, _named(name), N, 0)
    resets, _ = _same_rollout(on, off, steps)
    assert resets > 0                      # (episodes of 30 steps)
    on.close(); off.close()


@pytest.mark.parametrize("other", ["classic", "zero_fill"])
def test_poison_with_heavy_and_empty_teams(gpu_device, monkeypatch, other):
    """lying envs (>= 6 contacts, limit rows) beside free-falling ones (no rows), the workgroup's LDS pre-filled with NaN
    (SOLORL_POISON_LDS): the same bits as the classic kernel, and as the duo kernel over a zero fill -- neither wavefront reads a word
    across D, A or Z that the launch has not written.  (Termination is off, as the lying pose needs: no resets in this window.)"""
    cfg = _walk12(no_termination=True)
    nan = _env(monkeypatch, cfg, 6, 1, poison=NAN_WORD)
    ref = _env(monkeypatch, cfg, 6, 0) if other == "classic" else _env(monkeypatch, cfg, 6, 1, poison="0")
    _, first = _same_rollout(nan, ref, 40, air=AIR, lying=LYING)
    assert all(first[i] == 0 for i in AIR) and max(first[i] for i in LYING) >= 6, first
    nan.close(); ref.close()


def test_replayed_graph(gpu_device, monkeypatch):
    """three steps with two history levels captured in a HIP graph and replayed, against the classic kernel launched eagerly"""
    N = 5
    graphed, eager = _env(monkeypatch, _walk12(history=2), N, 1), _env(monkeypatch, _walk12(history=2), N, 0)
    assert torch.equal(graphed.reset(), eager.reset())
    g = torch.Generator(device="cuda:0"); g.manual_seed(5)
    acts = torch.rand(3, N, 12, device="cuda:0", generator=g) * 2 - 1
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up outside the capture (the kernels' first launch loads their code)
        graphed.step_inplace(acts[0]); eager.step_inplace(acts[0])
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    outs = []
    with torch.cuda.graph(graph):
        for k in range(3):
            o, r, d, _ = graphed.step_inplace(acts[k])
            outs.append((o.clone(), r.clone(), d.clone()))
    resets = 0
    for rep in range(14):                              # (42 steps: past the 25-step time limit, so a reset falls inside a replay)
        graph.replay()
        for k in range(3):
            o, r, d, _ = eager.step_inplace(acts[k])
            assert torch.equal(o, outs[k][0]) and torch.equal(r, outs[k][1]) and torch.equal(d, outs[k][2]), (rep, k)
            resets += int(d.sum())                     # (the classic kernel's done flags)
    torch.cuda.synchronize()
    assert resets > 0
    assert torch.equal(graphed.get_states().bytes(), eager.get_states().bytes())
    graphed.close(); eager.close()
