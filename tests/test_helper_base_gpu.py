"""The helper wavefront's base solve (duo_kernel_team, DESIGN section 4 "Helper wavefront": leg sum, base solve and leg rates on the
helper between barriers B and C, beside the main wavefront's leg rows) against the classic one-wavefront kernel (SOLORL_HELPER_WAVE=0),
bitwise, at the shapes and branches tests/test_helper_wave_gpu.py does not reach: other sub-step counts (the barriers per step follow
frame_skip), the URDF-inertia instantiations around the hand-off, a team without rows (the helper parks the null row) beside teams with
rows, and teams with 17 rows or more (the second row per lane of phase_finish_team).  Same seed, same actions: observations, rewards,
done flags, the info arrays, the applied torques, the episode accumulators and every env's state must be the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN_WORD = "0x7fc00000"
INFO = ("timeout", "success", "nan_reset", "episode_length", "episode_reward", "goals_reached",
        "dr_stand", "dr_joint_pose", "dr_torque", "dr_balance", "dr_progress")
AIR, LYING = (0, 4), (1, 5)             # envs of the N = 6 mixes: one of each kind in either workgroup (envs 0..3 | 4, 5, two idle teams)
# The lying pose, chosen on the CPU with the fp64 oracle (oracle.oracle_py.Oracle, set_caps(8, 4), termination disabled, seed 7, U(-1, 1)
# actions): base level at z = 0.020 / 0.025 m (the belly plate's corners are 0.025 m below the base origin), every leg folded to
# (HAA, HFE, KFE) = (0, +limit, -limit), at rest.  First sub-step: 16 primitives touch (12 at z = 0.025), capped, 8 limit candidates of
# which 4 get rows; after the first control step the oracle has 8 contacts solved (belly corners, feet, shoulders: mask 0x3aa300 /
# 0x0aaf00) and 2 / 1 limit rows -- 26 / 25 rows -- and still 6 to 8 contacts five steps later.
LYING_Z = (0.020, 0.025)


def _cfg(frame_skip=None, urdf=0, no_termination=False):
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    c = default_config(ROBOT_SOLO12, TASK_WALK); c.num_history_stack = 1; c.episode_length = 25
    if frame_skip is not None:
        c.frame_skip = frame_skip
    c.use_urdf_inertia = urdf
    if no_termination:                   # (a base below 0.05 m ends the episode: the lying envs would be reset by their first step)
        c.disable_termination = 1
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
    """after the reset: the `air` envs lifted to base z = 1.0 at rest, the `lying` envs laid on the ground (LYING_Z); both handles get
    the same rows"""
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
    state -> contacts per env after the first step"""
    N, A = a.nenvs, a.act_dim
    assert torch.equal(a.reset(), b.reset())
    if air or lying:
        _place(a, b, air, lying)
    g = torch.Generator(device="cuda:0"); g.manual_seed(seed)
    first = None
    for k in range(steps):
        act = torch.rand(N, A, device="cuda:0", generator=g) * 2 - 1
        oa, ra, da, ia = a.step_inplace(act)
        ob, rb, db, ib = b.step_inplace(act)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
        assert torch.equal(a._tau, b._tau), k
        for f in INFO:
            assert torch.equal(ia[f], ib[f]), (k, f)
        if k == 0:
            first = _contacts(a)
            assert first == _contacts(b)
    torch.cuda.synchronize()
    assert torch.equal(a._ep_stats, b._ep_stats)
    assert torch.equal(a.get_states().bytes(), b.get_states().bytes())
    for i in range(N):
        assert bytes(a.get_state(i)) == bytes(b.get_state(i)), i
    return first


@pytest.mark.parametrize("frame_skip", [1, 3])
def test_other_substep_counts(gpu_device, monkeypatch, frame_skip):
    """three barriers per sub-step and role: a count that did not follow frame_skip would hang or desynchronise the hand-offs"""
    on, off = _env(monkeypatch, _cfg(frame_skip), 5, 1), _env(monkeypatch, _cfg(frame_skip), 5, 0)
    _same_rollout(on, off, 30)
    on.close(); off.close()


def test_urdf_inertia(gpu_device, monkeypatch):
    """the UI = true instantiations of the front (helper) and the leg phase (main) on either side of the new hand-off"""
    on, off = _env(monkeypatch, _cfg(urdf=1), 9, 1), _env(monkeypatch, _cfg(urdf=1), 9, 0)
    _same_rollout(on, off, 30)
    on.close(); off.close()


def test_team_without_rows_beside_teams_with_rows(gpu_device, monkeypatch):
    """envs 0 and 4 fall freely from z = 1.0 (nothing touches, no joint at its limit): the helper's phase_base_lead parks their null
    row while the main wavefront parks the rows of the standing envs beside them"""
    on, off = _env(monkeypatch, _cfg(), 6, 1), _env(monkeypatch, _cfg(), 6, 0)
    first = _same_rollout(on, off, 10, air=AIR)
    last = _contacts(on)
    assert all(first[i] == 0 and last[i] == 0 for i in AIR), (first, last)
    assert any(first[i] > 0 for i in range(6) if i not in AIR), first
    on.close(); off.close()


def test_heavy_teams(gpu_device, monkeypatch):
    """envs 1 and 5 lie on the ground with folded legs: base and leg contacts capped, limit rows present, >= 17 rows -- the second
    row per lane in phase_finish_team, the heaviest hand-off from the helper's bc / hdr to the main wavefront"""
    cfg = _cfg(no_termination=True)
    on, off = _env(monkeypatch, cfg, 6, 1), _env(monkeypatch, cfg, 6, 0)
    first = _same_rollout(on, off, 10, lying=LYING)
    print("contacts per env after the first step:", first)
    assert max(first[i] for i in LYING) >= 6, first                  # >= 6 contacts: 18 rows without a single limit row
    on.close(); off.close()


def test_poison_with_heavy_and_empty_teams(gpu_device, monkeypatch):
    """helper on, the workgroup's LDS pre-filled with NaN and with zeros (SOLORL_POISON_LDS), lying and falling envs mixed: the same
    bits -- neither wavefront reads a word of the B-to-C hand-offs that the launch has not written"""
    cfg = _cfg(no_termination=True)
    nan, zero = _env(monkeypatch, cfg, 6, 1, poison=NAN_WORD), _env(monkeypatch, cfg, 6, 1, poison="0")
    first = _same_rollout(nan, zero, 10, air=AIR, lying=LYING)
    assert all(first[i] == 0 for i in AIR) and max(first[i] for i in LYING) >= 6, first
    nan.close(); zero.close()
