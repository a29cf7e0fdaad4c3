"""The duo kernel's split row finish (duo_kernel_team, DESIGN section 4 "Helper wavefront": behind barrier C the main wavefront finishes
rows 0..15 and the helper rows 16.., duo_finish_rows; barrier C2; then the sweep) against the classic one-wavefront kernel
(SOLORL_HELPER_WAVE=0), which runs phase_finish_team as it was.  Same seed, same actions: observations, rewards, done flags, the info
arrays, the applied torques, the episode accumulators and every env's state must be the same bits.

Shapes: N = 5 (a full workgroup, a ragged one, empty ones in the padded grid), frame_skip 1 and 4 (5 x frame_skip + 1 barriers per
role and step), envs lying on folded legs (8 contacts and limit rows: 17 rows or more, so the helper has rows to finish) beside
free-falling ones (no rows: every impulse position is zeroed, 0..15 by the main wavefront and 16..25 by the helper), walking envs
with resets, Solo8 on the treadmill; plain and under the LDS poison hook with a NaN fill against a zero fill; a replayed graph.
The fp64 kernels are classic ones and were not changed: their case holds them to hashes recorded with the parent commit's library
(tests/golden/make_golden_finish_split_f64.py)."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAN_WORD = "0x7fc00000"
INFO = ("timeout", "success", "nan_reset", "episode_length", "episode_reward", "goals_reached",
        "dr_stand", "dr_joint_pose", "dr_torque", "dr_balance", "dr_progress")
AIR, LYING = (0, 3), (1, 2, 4)          # N = 5: envs 0..3 in the first workgroup, env 4 beside three idle teams in the second
LYING_Z = (0.020, 0.025)                # the lying pose of tests/test_helper_base_gpu.py (chosen there with the fp64 oracle)


def _walk12(frame_skip, no_termination=True):
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    c = default_config(ROBOT_SOLO12, TASK_WALK); c.num_history_stack = 1; c.episode_length = 25
    c.frame_skip = frame_skip
    if no_termination:                   # (a base below 0.05 m ends the episode: the lying envs would be reset by their first step)
        c.disable_termination = 1
    return c


def _walk8_treadmill():
    from solorl_amd.config import config_from_dict, load_yaml, TASK_WALK
    c = config_from_dict(load_yaml(os.path.join(ROOT, "configs", "basic.yaml"))); c.task = TASK_WALK; c.episode_length = 30
    assert c.use_treadmill
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
    """after the reset: the `air` envs lifted to base z = 1.0 at rest, the `lying` envs laid on the ground with folded legs; both
    handles get the same rows"""
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


def _heavy_and_empty(first):
    # >= 6 contacts are 18 rows without a single limit row: the helper's lanes have rows to finish
    assert all(first[i] == 0 for i in AIR) and max(first[i] for i in LYING) >= 6, first


@pytest.mark.parametrize("frame_skip", [1, 4])
def test_lying_and_falling_envs_against_the_classic_kernel(gpu_device, monkeypatch, frame_skip):
    cfg = _walk12(frame_skip)
    on, off = _env(monkeypatch, cfg, 5, 1), _env(monkeypatch, cfg, 5, 0)
    _, first = _same_rollout(on, off, 20, air=AIR, lying=LYING)
    print("contacts per env after the first step:", first)
    _heavy_and_empty(first)
    on.close(); off.close()


@pytest.mark.parametrize("frame_skip", [1, 4])
def test_lying_and_falling_envs_under_the_lds_poison(gpu_device, monkeypatch, frame_skip):
    """NaN fill against zero fill, both on the duo kernel: neither wavefront reads a word between C and C2, nor the sweep behind it,
    that the launch has not written -- the rows a team does not have and the positions it leaves empty included"""
    cfg = _walk12(frame_skip)
    nan, zero = _env(monkeypatch, cfg, 5, 1, poison=NAN_WORD), _env(monkeypatch, cfg, 5, 1, poison="0")
    _, first = _same_rollout(nan, zero, 20, air=AIR, lying=LYING)
    _heavy_and_empty(first)
    nan.close(); zero.close()


@pytest.mark.parametrize("frame_skip", [1, 4])
def test_walking_envs_with_resets(gpu_device, monkeypatch, frame_skip):
    """the ordinary mix of row counts (every sweep variant a falling robot meets), with the time limit on: resets inside the window"""
    cfg = _walk12(frame_skip, no_termination=False)
    on, off = _env(monkeypatch, cfg, 5, 1), _env(monkeypatch, cfg, 5, 0)
    resets, _ = _same_rollout(on, off, 40)
    assert resets > 0
    on.close(); off.close()


@pytest.mark.parametrize("poison", [None, NAN_WORD])
def test_solo8_on_the_treadmill(gpu_device, monkeypatch, poison):
    """the other robot's lane map and row counts (two joints per leg: the third component of a leg is absent from every row)"""
    cfg = _walk8_treadmill()
    on = _env(monkeypatch, cfg, 5, 1, poison=poison)
    ref = _env(monkeypatch, cfg, 5, 0) if poison is None else _env(monkeypatch, cfg, 5, 1, poison="0")
    resets, _ = _same_rollout(on, ref, 60)
    assert resets > 0                      # (episodes of 30 steps)
    on.close(); ref.close()


def test_replayed_graph(gpu_device, monkeypatch):
    """three steps captured in a HIP graph and replayed, lying and falling envs mixed, against the classic kernel launched eagerly"""
    N, cfg = 5, _walk12(4)
    graphed, eager = _env(monkeypatch, cfg, N, 1), _env(monkeypatch, cfg, N, 0)
    assert torch.equal(graphed.reset(), eager.reset())
    _place(graphed, eager, AIR, LYING)
    g = torch.Generator(device="cuda:0"); g.manual_seed(5)
    acts = torch.rand(4, N, 12, device="cuda:0", generator=g) * 2 - 1
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up outside the capture (the kernels' first launch loads their code)
        graphed.step_inplace(acts[3]); eager.step_inplace(acts[3])
    torch.cuda.current_stream().wait_stream(side)
    first = _contacts(graphed)
    assert first == _contacts(eager)
    _heavy_and_empty(first)
    graph = torch.cuda.CUDAGraph()
    outs = []
    with torch.cuda.graph(graph):
        for k in range(3):
            o, r, d, _ = graphed.step_inplace(acts[k])
            outs.append((o.clone(), r.clone(), d.clone()))
    for rep in range(5):
        graph.replay()
        for k in range(3):
            o, r, d, _ = eager.step_inplace(acts[k])
            assert torch.equal(o, outs[k][0]) and torch.equal(r, outs[k][1]) and torch.equal(d, outs[k][2]), (rep, k)
    torch.cuda.synchronize()
    assert torch.equal(graphed.get_states().bytes(), eager.get_states().bytes())
    graphed.close(); eager.close()


def test_fp64_kernels_are_the_parents(gpu_device):
    """5 envs, 20 steps on the fp64 instantiation (a classic kernel: phase_finish_team, pgs_team_variant), lying and falling envs
    mixed: the hashes recorded with the parent commit's library"""
    spec = importlib.util.spec_from_file_location("make_golden_finish_split_f64", os.path.join(HERE, "golden", "make_golden_finish_split_f64.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = json.load(open(gen.FIXTURE))
    got = gen.run_case()
    assert got["contacts_first_step"] == want["contacts_first_step"]
    assert max(got["contacts_first_step"]) >= 6 and min(got["contacts_first_step"]) == 0
    assert got == want
