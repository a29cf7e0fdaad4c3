"""K control steps in one launch (include/solorl.h solorl_step_n, solorl_rollout) against K single launches, bitwise.

The per-step reference handle runs under SOLORL_POISON_LDS (every step_team call refills the team's LDS with NaN first); the K-step handle
runs without it, so a step inside a window that read LDS left over from the previous step would differ from the reference."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_WORD = "0x7fc00000"
INFO = ("timeout", "success", "nan_reset", "episode_length", "episode_reward", "goals_reached",
        "dr_stand", "dr_joint_pose", "dr_torque", "dr_balance", "dr_progress")


def _cfg(name):
    from solorl_amd.config import default_config, config_from_dict, load_yaml, ROBOT_SOLO8, ROBOT_SOLO12, TASK_STAND, TASK_WALK
    if name == "walk12":
        c = default_config(ROBOT_SOLO12, TASK_WALK); c.num_history_stack = 1; c.episode_length = 25
    elif name == "contact12_pd":
        c = config_from_dict(load_yaml(os.path.join(ROOT, "configs", "basic_contact.yaml")))
    elif name == "basic8_treadmill":
        c = config_from_dict(load_yaml(os.path.join(ROOT, "configs", "basic.yaml"))); c.episode_length = 30
    elif name == "stand8":
        c = default_config(ROBOT_SOLO8, TASK_STAND); c.num_history_stack = 1; c.episode_length = 30
    elif name == "pointgoal12":
        c = config_from_dict(load_yaml(os.path.join(ROOT, "configs", "basic12.yaml"))); c.episode_length = 30
    elif name == "walk12_f64":
        c = default_config(ROBOT_SOLO12, TASK_WALK); c.num_history_stack = 1; c.episode_length = 25; c.precision = 1
    elif name == "walk12_hist3":
        c = default_config(ROBOT_SOLO12, TASK_WALK); c.num_history_stack = 3; c.episode_length = 25
    else:
        raise KeyError(name)
    return c


def _pair(monkeypatch, cfg, N, seed=7):
    """(reference handle under the LDS poison, K-step handle without it), same seed, both reset."""
    from solorl_amd.vec_env import SoloVecEnv
    dev = torch.device("cuda:0")
    monkeypatch.setenv("SOLORL_POISON_LDS", NAN_WORD)
    ref = SoloVecEnv(cfg, N, device=dev, seed=seed, applied_torque=True)
    monkeypatch.delenv("SOLORL_POISON_LDS")
    cand = SoloVecEnv(cfg, N, device=dev, seed=seed, applied_torque=True)
    assert torch.equal(ref.reset(), cand.reset())
    return ref, cand


def _per_step(env, actions):
    """K x step_inplace -> stacked copies of every per-step output"""
    rows = {k: [] for k in ("obs", "rew", "done", "applied_torque") + INFO}
    for k in range(actions.shape[0]):
        o, r, d, info = env.step_inplace(actions[k].contiguous())
        rows["obs"].append(o.clone()); rows["rew"].append(r.clone()); rows["done"].append(d.clone())
        rows["applied_torque"].append(env._tau.clone())
        for f in INFO:
            rows[f].append(info[f].clone())
    return {k: torch.stack(v) for k, v in rows.items()}


def _same_state(a, b, envs):
    for i in envs:
        assert bytes(a.get_state(i)) == bytes(b.get_state(i)), i


def _open_loop(monkeypatch, name, N, windows, burn_in=0, seed=7):
    ref, cand = _pair(monkeypatch, _cfg(name), N, seed)
    assert cand.get_property("step_n_one_launch") == 1
    g = torch.Generator(device="cuda:0"); g.manual_seed(11)
    A = ref.act_dim
    for _ in range(burn_in):
        a = torch.rand(N, A, device="cuda:0", generator=g) * 2 - 1
        ref.step_inplace(a); cand.step_inplace(a)
    fired = 0
    for K in windows:
        acts = torch.rand(K, N, A, device="cuda:0", generator=g) * 3 - 1.5        # (beyond +-1: the clip too)
        want = _per_step(ref, acts)
        o, r, d, info = cand.step_n_inplace(acts)
        assert torch.equal(o, want["obs"]), (name, K)
        assert torch.equal(r, want["rew"]) and torch.equal(d, want["done"]), (name, K)
        assert torch.equal(info["applied_torque"], want["applied_torque"]), (name, K)
        for f in INFO:
            assert torch.equal(info[f], want[f]), (name, K, f)
        fired += int(d.sum())
    torch.cuda.synchronize()
    assert fired > 0, name                               # episodes ended (and auto-reset) inside the windows
    assert torch.equal(ref._ep_stats, cand._ep_stats)
    _same_state(ref, cand, sorted({0, 1, N // 2, N - 2, N - 1}))
    ref.close(); cand.close()


@pytest.mark.parametrize("name,N", [("walk12", 67), ("contact12_pd", 64), ("basic8_treadmill", 40), ("stand8", 33), ("pointgoal12", 48),
                                    ("walk12_f64", 37), ("walk12_hist3", 29)])
def test_step_n_equals_k_single_steps_bitwise(gpu_device, monkeypatch, name, N):
    """K = 1 and K = 37 (and 37 again: episode length 50 ends inside it): observations, rewards, done flags, the 11 info fields and the
    applied torques of every step, then the episode accumulators and the full state of the first, middle and last envs."""
    _open_loop(monkeypatch, name, N, (1, 37, 37))


def test_step_n_full_size_window_bitwise(gpu_device, monkeypatch):
    """The bench workload: 4096 Solo12 walk envs after the 450-step burn-in, one window of K = 400."""
    _open_loop(monkeypatch, "walk12", 4096, (400,), burn_in=450)


def _policy(dev, O, A, seed=3):
    from solorl_amd.ppo import Policy
    from solorl_amd.vec_env import Box
    torch.manual_seed(seed)
    pol = Policy((O,), Box(-np.ones(A), np.ones(A)), None, {"hidden_size": 64}).to(dev)
    with torch.no_grad():
        pol.pi_dist.logstd.normal_(0, 0.3)
        for p in pol.parameters():
            if p.dim() == 1 and p is not pol.pi_dist.logstd:
                p.normal_(0, 0.1)
    return pol


def _closed_ref(env, P, a0, noise, K, pal):
    """K x step_act_inplace (the last one a plain step unless pal), each step driven by the action the previous one produced"""
    N, A, dev = env.nenvs, env.act_dim, a0.device
    R = K + pal
    act = torch.full((R, N, A), 7.0, device=dev); act[0] = a0
    val, lp = torch.full((R, N), 7.0, device=dev), torch.full((R, N), 7.0, device=dev)
    obs, rew, done = [], [], []
    for k in range(K):
        if k + 1 < K or pal:
            o, r, d, _ = env.step_act_inplace(act[k], P, None if noise is None else noise[k + 1].contiguous(), val[k + 1], act[k + 1], lp[k + 1])
        else:
            o, r, d, _ = env.step_inplace(act[k])
        obs.append(o.clone()); rew.append(r.clone()); done.append(d.clone())
    return dict(obs=torch.stack(obs), rew=torch.stack(rew), done=torch.stack(done), act=act, val=val, lp=lp)


def _closed_cand(env, P, a0, noise, K, pal):
    N, A, dev = env.nenvs, env.act_dim, a0.device
    R = K + pal
    act = torch.full((R, N, A), 7.0, device=dev); act[0] = a0
    val, lp = torch.full((R, N), 7.0, device=dev), torch.full((R, N), 7.0, device=dev)
    o, r, d, _ = env.rollout_inplace(act, P, None if noise is None else noise[:R].contiguous(), val, lp, policy_after_last=bool(pal))
    return dict(obs=o.clone(), rew=r.clone(), done=d.clone(), act=act, val=val, lp=lp)


def _same_closed(x, y, what):
    for k in ("obs", "rew", "done", "act", "val", "lp"):
        assert torch.equal(x[k], y[k]), (what, k)


@pytest.mark.parametrize("with_noise,pal", [(True, 1), (True, 0), (False, 1), (False, 0)])
def test_rollout_equals_k_step_act_bitwise(gpu_device, monkeypatch, with_noise, pal):
    """solorl_rollout against K x solorl_step_act closed as in tests/test_train_gpu.py::test_step_act_equals_step_then_policy_act:
    observations, rewards, done flags and the policy's value, action and log-prob of every row, bitwise (the same kernel code computes
    both); rows the call must not touch keep their fill value."""
    from solorl_amd.ppo.fused import policy_params
    ref, cand = _pair(monkeypatch, _cfg("walk12"), 67, seed=5)
    P = policy_params(_policy(gpu_device, 76, 12))
    assert cand.rollout_supported(P)
    g = torch.Generator(device="cuda:0"); g.manual_seed(13)
    a0 = torch.rand(67, 12, device="cuda:0", generator=g) * 2 - 1
    for K in (1, 30):
        noise = torch.randn(K + 1, 67, 12, device="cuda:0", generator=g) if with_noise else None
        want, got = _closed_ref(ref, P, a0, noise, K, pal), _closed_cand(cand, P, a0, noise, K, pal)
        _same_closed(want, got, (K, with_noise, pal))
        assert (got["val"][0] == 7.0).all() and (got["lp"][0] == 7.0).all()
        if not pal:
            assert K == 1 or not (got["act"][K - 1] == 7.0).any()
        a0 = got["act"][K] if pal else torch.rand(67, 12, device="cuda:0", generator=g) * 2 - 1
    torch.cuda.synchronize()
    assert torch.equal(ref._ep_stats, cand._ep_stats)
    _same_state(ref, cand, (0, 33, 66))
    ref.close(); cand.close()


def test_two_rollout_windows_equal_one(gpu_device):
    """Windows of K1 and K2 (the first evaluating the policy after its last step) = one window of K1 + K2."""
    from solorl_amd.ppo.fused import policy_params
    from solorl_amd.vec_env import SoloVecEnv
    dev = gpu_device
    e1, e2 = SoloVecEnv(_cfg("walk12"), 67, device=dev, seed=9), SoloVecEnv(_cfg("walk12"), 67, device=dev, seed=9)
    assert torch.equal(e1.reset(), e2.reset())
    P = policy_params(_policy(dev, 76, 12, seed=4))
    g = torch.Generator(device="cuda:0"); g.manual_seed(17)
    K1, K2 = 13, 21
    noise = torch.randn(K1 + K2 + 1, 67, 12, device="cuda:0", generator=g)
    a0 = torch.rand(67, 12, device="cuda:0", generator=g) * 2 - 1
    one = _closed_cand(e1, P, a0, noise, K1 + K2, 1)
    w1 = _closed_cand(e2, P, a0, noise, K1, 1)
    w2 = _closed_cand(e2, P, w1["act"][K1], noise[K1:], K2, 1)
    assert int(one["done"].sum()) > 0
    assert torch.equal(one["obs"], torch.cat([w1["obs"], w2["obs"]])) and torch.equal(one["rew"], torch.cat([w1["rew"], w2["rew"]]))
    assert torch.equal(one["done"], torch.cat([w1["done"], w2["done"]]))
    for k in ("act", "val", "lp"):
        assert torch.equal(one[k][1:], torch.cat([w1[k][1:], w2[k][1:]])), k
    e1.close(); e2.close()


@pytest.mark.parametrize("var,val", [("SOLORL_TEAM", "0"), ("SOLORL_SORT", "1")])
def test_step_n_without_a_k_step_kernel_issues_single_steps(gpu_device, monkeypatch, var, val):
    """Lane mode and contact-count sorting have no one-launch form: step_n issues K ordinary steps (the same results), the property says
    0, and rollout_inplace refuses -- decided from the handle, not from the environment at call time."""
    from solorl_amd import _native
    from solorl_amd.ppo.fused import policy_params
    from solorl_amd.vec_env import SoloVecEnv
    monkeypatch.setenv(var, val)
    cfg = _cfg("walk12")
    ea, eb = SoloVecEnv(cfg, 36, device=gpu_device, seed=2, applied_torque=True), SoloVecEnv(cfg, 36, device=gpu_device, seed=2, applied_torque=True)
    monkeypatch.delenv(var)
    assert ea.get_property("step_n_one_launch") == 0 and eb.get_property("step_n_one_launch") == 0
    assert torch.equal(ea.reset(), eb.reset())
    g = torch.Generator(device="cuda:0"); g.manual_seed(3)
    for K in (1, 30):
        acts = torch.rand(K, 36, 12, device="cuda:0", generator=g) * 2 - 1
        want = _per_step(ea, acts)
        o, r, d, info = eb.step_n_inplace(acts)
        assert torch.equal(o, want["obs"]) and torch.equal(r, want["rew"]) and torch.equal(d, want["done"])
        assert torch.equal(info["applied_torque"], want["applied_torque"])
        for f in INFO:
            assert torch.equal(info[f], want[f]), f
    assert torch.equal(ea._ep_stats, eb._ep_stats)
    P = policy_params(_policy(gpu_device, 76, 12))
    assert not eb.rollout_supported(P)
    with pytest.raises(_native.SoloRLError, match="team-mode"):
        eb.rollout_inplace(torch.zeros(3, 36, 12, device=gpu_device), P, None, torch.zeros(3, 36, device=gpu_device),
                           torch.zeros(3, 36, device=gpu_device), policy_after_last=True)
    ea.close(); eb.close()


def test_rollout_refuses_f64_and_wide_observations_and_step_n_needs_reset(gpu_device):
    from solorl_amd import _native
    from solorl_amd.ppo.fused import policy_params
    from solorl_amd.vec_env import SoloVecEnv
    for name, O, msg in (("walk12_f64", 76, "team-mode"), ("walk12_hist3", 152, "at most 88")):
        env = SoloVecEnv(_cfg(name), 8, device=gpu_device, seed=1)
        assert env.obs_dim == O
        P = policy_params(_policy(gpu_device, O, 12))
        assert not env.rollout_supported(P)
        env.reset()
        with pytest.raises(_native.SoloRLError, match=msg):
            env.rollout_inplace(torch.zeros(2, 8, 12, device=gpu_device), P, None, torch.zeros(2, 8, device=gpu_device),
                                torch.zeros(2, 8, device=gpu_device))
        env.close()
    env = SoloVecEnv(_cfg("walk12"), 8, device=gpu_device, seed=1)
    with pytest.raises(_native.SoloRLError, match="reset"):
        env.step_n(torch.zeros(3, 8, 12, device=gpu_device))
    env.close()


@pytest.mark.parametrize("chunk", [12, 5])
def test_graphed_rollout_in_windows(gpu_device, chunk):
    """GraphedRollout(chunk=K) at T = 12 (K = 5: windows 5, 5, 2): the stored values / log-probs are the policy's on the stored rows, the
    stored actions replayed on a fresh handle reproduce the stored observations, rewards and masks bitwise, and a second replay of the
    graph continues the episodes."""
    from solorl_amd.ppo import Policy, RolloutStorage
    from solorl_amd.ppo.graphs import GraphedRollout
    from solorl_amd.vec_env import Box, SoloVecEnv
    dev = gpu_device
    N, T = 256, 12
    cfg = _cfg("walk12")
    torch.manual_seed(0)
    pol = Policy((76,), Box(-np.ones(12), np.ones(12)), None, {"hidden_size": 64}).to(dev)
    env = SoloVecEnv(cfg, N, device=dev, seed=3)
    st = RolloutStorage(T, N, (76,), 12, dev)
    st.obs[0].copy_(env.reset())
    with torch.no_grad():
        pol.act(st.obs[0])
    roll = GraphedRollout(env, pol, st, T, chunk=chunk)
    env2 = SoloVecEnv(cfg, N, device=dev, seed=3)
    assert torch.equal(env2.reset(), st.obs[0])
    ended = 0
    for rep in range(2):
        if rep:
            st.reset()
        roll()
        torch.cuda.synchronize()
        assert roll.windows == [min(chunk, T - t0) for t0 in range(0, T, chunk)]
        g = {k: getattr(st, k).clone() for k in ("obs", "actions", "action_log_probs", "value_preds", "rewards", "masks")}
        with torch.no_grad():
            for t in range(T):
                v, lp, _ = pol.evaluate_actions(g["obs"][t], g["actions"][t])
                assert torch.allclose(v, g["value_preds"][t], atol=1e-5) and torch.allclose(lp, g["action_log_probs"][t], atol=1e-4), (rep, t)
        for t in range(T):                    # env2 continues from where the previous replay left it
            o, r, d, _ = env2.step_inplace(g["actions"][t].contiguous())
            assert torch.equal(o, g["obs"][t + 1]), (rep, t)
            assert torch.equal(r.view(-1), g["rewards"][t].view(-1)) and torch.equal(1.0 - d.float(), g["masks"][t + 1].view(-1)), (rep, t)
            ended += int(d.sum())
    assert ended > 0                          # (episode length 25 < 2 T)
    env.close(); env2.close()
