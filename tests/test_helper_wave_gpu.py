"""The step kernel's helper wavefront (duo_kernel_team, DESIGN section 4 "Helper wavefront") against the classic one-wavefront kernel
(SOLORL_HELPER_WAVE=0), bitwise: the collision front moves to a second wavefront, no arithmetic changes, so observations, rewards, done
flags, the info arrays, the applied torques, the episode accumulators and the full state of every env must be the same bits."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_WORD = "0x7fc00000"
INFO = ("timeout", "success", "nan_reset", "episode_length", "episode_reward", "goals_reached",
        "dr_stand", "dr_joint_pose", "dr_torque", "dr_balance", "dr_progress")


def _cfg(name):
    from solorl_amd.config import default_config, config_from_dict, load_yaml, ROBOT_SOLO12, TASK_WALK, TASK_POINTGOAL, CONTROL_PD
    if name == "walk12":
        c = default_config(ROBOT_SOLO12, TASK_WALK); c.num_history_stack = 1; c.episode_length = 25
    elif name == "walk8_treadmill":
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


def _same_rollout(a, b, steps, seed=11):
    """the same seeded U(-1, 1) actions on both handles: every per-step output of every step, then the accumulators and every env's state"""
    N, A = a.nenvs, a.act_dim
    assert torch.equal(a.reset(), b.reset())
    g = torch.Generator(device="cuda:0"); g.manual_seed(seed)
    resets = 0
    for k in range(steps):
        act = torch.rand(N, A, device="cuda:0", generator=g) * 2 - 1
        oa, ra, da, ia = a.step_inplace(act)
        ob, rb, db, ib = b.step_inplace(act)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), k
        assert torch.equal(a._tau, b._tau), k
        for f in INFO:
            assert torch.equal(ia[f], ib[f]), (k, f)
        resets += int(da.sum())
    torch.cuda.synchronize()
    assert torch.equal(a._ep_stats, b._ep_stats)
    for i in range(N):
        assert bytes(a.get_state(i)) == bytes(b.get_state(i)), i
    return resets


@pytest.mark.parametrize("name,N,steps", [("walk12", 67, 80),             # 17 groups, the last ragged, and the padded grid's empty ones
                                          ("walk8_treadmill", 5, 80),
                                          ("pointgoal12_pd", 9, 60),      # limit rows; quiet teams
                                          ("walk12", 1, 80),              # one team valid
                                          ("walk12", 4, 80)])             # one full group
def test_helper_wave_equals_classic_kernel_bitwise(gpu_device, monkeypatch, name, N, steps):
    on, off = _env(monkeypatch, _cfg(name), N, 1), _env(monkeypatch, _cfg(name), N, 0)
    resets = _same_rollout(on, off, steps)
    if (name, N) == ("walk12", 67):
        assert resets > 0
    on.close(); off.close()


def test_helper_wave_reads_no_lds_before_it_is_written(gpu_device, monkeypatch):
    """helper on, the workgroup's LDS pre-filled with NaN and with zeros (SOLORL_POISON_LDS): same bits -- neither wavefront reads what
    the launch has not written, and the hand-offs between the two are behind their barriers"""
    nan, zero = _env(monkeypatch, _cfg("walk12"), 67, 1, poison=NAN_WORD), _env(monkeypatch, _cfg("walk12"), 67, 1, poison="0")
    assert _same_rollout(nan, zero, 120) > 0
    nan.close(); zero.close()


def test_helper_wave_in_a_replayed_graph(gpu_device, monkeypatch):
    """three steps captured in a HIP graph and replayed (what the benchmark does) against the same three steps launched eagerly"""
    N = 67
    graphed, eager = _env(monkeypatch, _cfg("walk12"), N, 1), _env(monkeypatch, _cfg("walk12"), N, 1)
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
    for rep in range(2):
        graph.replay()
        for k in range(3):
            o, r, d, _ = eager.step_inplace(acts[k])
            assert torch.equal(o, outs[k][0]) and torch.equal(r, outs[k][1]) and torch.equal(d, outs[k][2]), (rep, k)
    torch.cuda.synchronize()
    for i in range(N):
        assert bytes(graphed.get_state(i)) == bytes(eager.get_state(i)), i
    graphed.close(); eager.close()


def test_helper_wave_is_refused_where_it_cannot_run(gpu_device, monkeypatch):
    """SOLORL_HELPER_WAVE=1 beyond one workgroup per SIMD, for fp64, lane mode or sorted storage: an error at create, not a silent no"""
    from solorl_amd import _native
    from solorl_amd.vec_env import SoloVecEnv
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    cfg64 = _cfg("walk12"); cfg64.precision = 1
    monkeypatch.setenv("SOLORL_HELPER_WAVE", "1")
    for cfg, N, extra in ((_cfg("walk12"), 4 * simds + 1, None), (cfg64, 8, None), (_cfg("walk12"), 8, ("SOLORL_TEAM", "0")),
                          (_cfg("walk12"), 8, ("SOLORL_SORT", "1"))):
        if extra:
            monkeypatch.setenv(*extra)
        with pytest.raises(_native.SoloRLError, match="SOLORL_HELPER_WAVE"):
            SoloVecEnv(cfg, N, device=torch.device("cuda:0"), seed=1)
        if extra:
            monkeypatch.delenv(extra[0])
    monkeypatch.delenv("SOLORL_HELPER_WAVE")
    big = SoloVecEnv(_cfg("walk12"), 4 * simds + 1, device=torch.device("cuda:0"), seed=1)      # the default above the size rule: classic
    assert big.get_property("helper_wave") == 0
    big.close()
