"""The policy kernels with a critic width of their own (csrc/solorl_ppo.hip: solorl_policy_act_critic, solorl_ppo_grad_stage1_critic /
stage2_critic, solorl_ppo_clip_adam on both widths) against PyTorch, with the bounds of the symmetric kernels' tests in
tests/test_train_gpu.py, and GraphedPPO / GraphedRollout on their kernel paths with an asymmetric policy."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPES = [(38, 58, 12), (41, 58, 12), (76, 96, 12), (30, 50, 8), (33, 50, 8), (60, 80, 8)]


def _random_policy(O, OC, A, seed=0):
    from solorl_amd.ppo import Policy
    from solorl_amd.vec_env import Box
    torch.manual_seed(seed)
    pol = Policy((O,), Box(-np.ones(A), np.ones(A)), None, {"hidden_size": 64}, critic_obs_dim=OC).to(DEV)
    with torch.no_grad():
        pol.pi_dist.logstd.normal_(0, 0.3)
        for p in pol.parameters():
            if p.dim() == 1 and p is not pol.pi_dist.logstd:
                p.normal_(0, 0.1)                   # non-zero biases
    return pol


@pytest.mark.parametrize("O,OC,A", SHAPES)
def test_policy_act_critic_kernel_matches_torch(gpu_device, O, OC, A):
    """solorl_policy_act_critic (one launch) == Policy.act_into with critic_inputs, 1000 rows (ragged), with noise and deterministic;
    the bounds of test_policy_act_kernel_matches_torch"""
    from solorl_amd import _native
    from solorl_amd.ppo.fused import policy_act, policy_params, policy_kernels_supported
    pol = _random_policy(O, OC, A)
    assert policy_kernels_supported(pol)
    P = policy_params(pol)
    assert P.critic_obs_dim == OC
    n = 1000
    obs, cobs = torch.randn(n, O, device=DEV), torch.randn(n, OC, device=DEV)
    for noise in (torch.randn(n, A, device=DEV), None):
        v0, a0, l0 = torch.empty(n, 1, device=DEV), torch.empty(n, A, device=DEV), torch.empty(n, 1, device=DEV)
        pol.act_into(obs, v0, a0, l0, noise=noise if noise is not None else torch.zeros(n, A, device=DEV), critic_inputs=cobs)
        v1, a1, l1 = torch.full((n, 1), 7.0, device=DEV), torch.full((n, A), 7.0, device=DEV), torch.full((n, 1), 7.0, device=DEV)
        policy_act(P, obs, noise, v1, a1, l1, critic_obs=cobs)
        assert torch.allclose(v0, v1, rtol=1e-4, atol=1e-5), (v0 - v1).abs().max().item()
        assert torch.allclose(a0, a1, rtol=1e-4, atol=1e-5), (a0 - a1).abs().max().item()
        assert torch.allclose(l0, l1, rtol=1e-4, atol=1e-4), (l0 - l1).abs().max().item()
    # the symmetric entry point refuses this policy; a shape that is not built keeps the PyTorch path
    with pytest.raises(_native.SoloRLError, match="critic_obs_dim must be 0"):
        _native.check(_native.lib().solorl_policy_act(C.byref(P), obs.data_ptr(), None, n, v1.data_ptr(), a1.data_ptr(), l1.data_ptr(), 0, _native.stream(DEV)))
    assert not policy_kernels_supported(_random_policy(O, OC + 4, A))


@pytest.mark.parametrize("O,OC,A,clipped", [(76, 96, 12, True), (33, 50, 8, False)])
def test_minibatch_grad_kernels_match_autograd(gpu_device, O, OC, A, clipped):
    """MiniBatchGrad on the _critic stages against loss.backward(): 16 x 128 rows, a mini-batch of 1024 at offset 512; every element
    of the bucket overwritten; the bounds of _check_minibatch_grad (rtol 2e-3, atol 2e-5 x the largest gradient, its loss bounds)"""
    from solorl_amd.ppo import RolloutStorage
    from solorl_amd.ppo import dist as D
    from solorl_amd.ppo.fused import MiniBatchGrad
    T, N, m, offset = 16, 128, 1024, 512
    clip, vc, ec = 0.1, 0.5, 0.01
    pol = _random_policy(O, OC, A, seed=1)
    st = RolloutStorage(T, N, (O,), A, DEV, critic_obs_dim=OC)
    torch.manual_seed(2)
    st.obs.normal_(); st.critic_obs.normal_(); st.actions.normal_(); st.value_preds.normal_(); st.returns.normal_()
    n = T * N
    flat = lambda x: x.reshape(n, *x.shape[2:])
    with torch.no_grad():                      # old log-probs near the current ones, every ratio 1e-3 away from the clip boundaries
        _, lp, _ = pol.evaluate_actions(flat(st.obs[:-1]), flat(st.actions), critic_inputs=flat(st.critic_obs[:-1]))
        noise = 0.15 * torch.randn_like(lp)
        for b in (1.0 - clip, 1.0 + clip):
            near = (torch.exp(-noise) - b).abs() < 1e-3
            noise = torch.where(near, noise + 0.01, noise)
        st.action_log_probs.copy_((lp + noise).view(T, N, 1))
    adv = torch.randn(n, 1, device=DEV)
    perm = torch.randperm(n, device=DEV)
    off = torch.full((), offset, dtype=torch.long, device=DEV)
    bucket = D.FlatGradBucket(pol.parameters())
    mb = MiniBatchGrad(pol, st, m, clip, vc, ec, clipped, perm, off, adv)
    assert mb.OC == OC and mb.cxt0 is not None
    bucket.flat.fill_(123.0)                    # every gradient element must be overwritten
    mb()
    g_kernel = bucket.flat.clone()
    assert not bool((g_kernel == 123.0).any())
    vl_k, al_k, ent_k = mb.losses(1)
    idx = perm[offset:offset + m]
    obs_b, cobs_b, act_b = flat(st.obs[:-1])[idx], flat(st.critic_obs[:-1])[idx], flat(st.actions)[idx]
    vpred_b, ret_b, old_b, adv_b = flat(st.value_preds[:-1])[idx], flat(st.returns[:-1])[idx], flat(st.action_log_probs)[idx], adv[idx]
    values, logp, entropy = pol.evaluate_actions(obs_b, act_b, critic_inputs=cobs_b)
    ratio = torch.exp(logp - old_b)
    al = -torch.min(ratio * adv_b, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv_b).mean()
    if clipped:
        v_clipped = vpred_b + (values - vpred_b).clamp(-clip, clip)
        vl = 0.5 * torch.max((values - ret_b).pow(2), (v_clipped - ret_b).pow(2)).mean()
    else:
        vl = 0.5 * (ret_b - values).pow(2).mean()
    bucket.zero()
    (vl * vc + al - entropy * ec).backward()
    g_ref = bucket.flat
    assert (ratio < 1 - clip).any() and (ratio > 1 + clip).any()
    scale = g_ref.abs().max().item()
    print("max |gradient difference| %.3g (largest gradient %.3g)" % ((g_kernel - g_ref).abs().max().item(), scale))
    assert torch.allclose(g_kernel, g_ref, rtol=2e-3, atol=2e-5 * scale), ((g_kernel - g_ref).abs().max().item(), scale)
    assert abs(vl_k - vl.item()) < 1e-4 * max(1.0, abs(vl.item())) and abs(al_k - al.item()) < 1e-5 + 1e-4 * abs(al.item())
    assert abs(ent_k - entropy.item()) < 1e-5
    # the work arrays: the actor's gathered rows in xt0, the critic's in its own (tiles [row / 32][unit][32])
    xt0 = mb.buf["xt0"].reshape(m // 32, O, 32).permute(0, 2, 1).reshape(m, O)
    cxt0 = mb.cxt0.reshape(m // 32, OC, 32).permute(0, 2, 1).reshape(m, OC)
    assert torch.equal(xt0, obs_b) and torch.equal(cxt0, cobs_b)


def test_clip_adam_kernel_on_both_widths_matches_torch(gpu_device):
    """solorl_ppo_clip_adam at (76, 96, 12) == clip_grad_norm_ + torch.optim.Adam.step, the bounds of test_clip_adam_kernel_matches_torch"""
    from solorl_amd.ppo import RolloutStorage
    from solorl_amd.ppo import dist as D
    from solorl_amd.ppo.fused import ClipAdam, MiniBatchGrad
    O, OC, A = 76, 96, 12
    for wd, max_norm in ((0.0, 0.5), (1e-3, None)):
        pol_a = _random_policy(O, OC, A, seed=9)
        pol_b = copy.deepcopy(pol_a)
        st = RolloutStorage(4, 64, (O,), A, DEV, critic_obs_dim=OC)
        bucket = D.FlatGradBucket(pol_a.parameters())
        off = torch.zeros((), dtype=torch.long, device=DEV)
        mb = MiniBatchGrad(pol_a, st, 64, 0.1, 0.5, 0.01, True, torch.arange(256, device=DEV), off, torch.zeros(256, 1, device=DEV))
        lr = torch.tensor(1e-3, device=DEV)
        ca = ClipAdam(mb, lr, max_norm, weight_decay=wd, offset=off, offset_increment=64)
        opt = torch.optim.Adam(pol_b.parameters(), lr=1e-3, weight_decay=wd)
        g = torch.Generator(device=DEV).manual_seed(1)
        for it in range(5):
            if it == 3:
                lr.fill_(4e-4)
                for grp in opt.param_groups:
                    grp["lr"] = 4e-4
            flat = torch.randn(bucket.flat.shape, device=DEV, generator=g) * (3.0 if it % 2 else 0.01)     # above and below the clip norm
            bucket.flat.copy_(flat)
            o = 0
            for p in pol_b.parameters():
                p.grad = flat[o:o + p.numel()].view_as(p).clone(); o += p.numel()
            ca()
            if max_norm is not None:
                torch.nn.utils.clip_grad_norm_(pol_b.parameters(), max_norm)
            opt.step()
            va = torch.cat([p.detach().flatten() for p in pol_a.parameters()])
            vb = torch.cat([p.detach().flatten() for p in pol_b.parameters()])
            assert torch.allclose(va, vb, rtol=1e-5, atol=2e-7), (it, (va - vb).abs().max().item())
        assert off.item() == 5 * 64 and ca.step.item() == 5.0


def test_hip_graph_update_on_the_kernel_path_matches_eager(gpu_device):
    """as test_hip_graph_update_with_the_minibatch_kernel_matches_eager, on an asymmetric policy (76, 96, 12)"""
    from solorl_amd.ppo import PPO, RolloutStorage
    from solorl_amd.ppo.graphs import GraphedPPO
    T, N, O, OC, A = 16, 128, 76, 96, 12
    torch.manual_seed(0)
    st = RolloutStorage(T, N, (O,), A, DEV, critic_obs_dim=OC)
    st.obs.normal_(); st.critic_obs.normal_(); st.actions.normal_(); st.rewards.normal_(); st.value_preds.normal_()
    st.action_log_probs.normal_().mul_(0.1).sub_(10)
    st.masks.copy_((torch.rand_like(st.masks) > 0.05).float())
    st.compute_returns(torch.randn(N, 1, device=DEV), True, 0.99, 0.95)
    pol_a = _random_policy(O, OC, A, seed=4)
    pol_b = copy.deepcopy(pol_a)
    eager = PPO(pol_a, 0.1, 2, 512, 0.5, 0.01, lr=1e-3, max_grad_norm=0.5)
    graph = GraphedPPO(pol_b, 0.1, 2, 512, 0.5, 0.01, lr=1e-3, max_grad_norm=0.5)
    assert graph.fused_mlp
    for it in range(2):
        torch.manual_seed(5 + it); la = eager.update(st)
        torch.manual_seed(5 + it); lb = graph.update(st)
        assert graph._mb is not None and graph._mb.OC == OC and graph._ca is not None
        assert np.allclose(la, lb, rtol=1e-4, atol=1e-5), (la, lb)
        va = torch.cat([p.detach().flatten() for p in pol_a.parameters()])
        vb = torch.cat([p.detach().flatten() for p in pol_b.parameters()])
        assert ((va - vb).norm() / va.norm()).item() < 1e-3 and (va - vb).abs().max().item() < 5e-3


def test_graphed_rollout_on_the_kernel_path(gpu_device):
    """GraphedRollout over 8 steps of 64 envs, Solo12 walk with one history level (76, 96, 12): one policy launch per step
    (solorl_policy_act_critic) plus the env's; the stored values equal get_value of the stored critic rows (1e-5), the stored log-probs
    evaluate_actions of the stored actor rows (1e-4)"""
    from solorl_amd import _native
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.ppo import RolloutStorage
    from solorl_amd.ppo.graphs import GraphedRollout
    from solorl_amd.vec_env import SoloVecEnv
    N, T = 64, 8
    cfg = default_config(ROBOT_SOLO12, TASK_WALK); cfg.num_history_stack = 1
    env = SoloVecEnv(cfg, N, device=DEV, seed=3, critic_obs=True)
    env.set_obs_noise(dict(joint_pos=0.05, joint_vel=1.0))
    pol = _random_policy(env.obs_dim, env.critic_obs_dim, 12, seed=2)
    st = RolloutStorage(T, N, (env.obs_dim,), 12, DEV, critic_obs_dim=env.critic_obs_dim)
    st.obs[0].copy_(env.reset())
    st.critic_obs[0].copy_(env.last_critic_obs)
    calls = []
    real = _native.lib()

    class Rec:
        def __getattr__(self, name):
            f = getattr(real, name)
            if not name.startswith("solorl_"):
                return f

            def call(*a):
                calls.append(name)
                return f(*a)
            return call
    _native._LIB = Rec()
    try:
        roll = GraphedRollout(env, pol, st, T)
        roll()
    finally:
        _native._LIB = real
    torch.cuda.synchronize()
    assert not roll.step_act and calls.count("solorl_policy_act_critic") == T and "solorl_policy_act" not in calls
    with torch.no_grad():
        for t in range(T):
            v = pol.get_value(None, critic_inputs=st.critic_obs[t])
            _, lp, _ = pol.evaluate_actions(st.obs[t], st.actions[t], critic_inputs=st.critic_obs[t])
            assert torch.allclose(v, st.value_preds[t], atol=1e-5) and torch.allclose(lp, st.action_log_probs[t], atol=1e-4), t
    assert bool((st.critic_obs[1:, :, 76:] != 0).any()) and bool((st.obs[1:] != st.critic_obs[1:, :, :76]).any())
    env.close()
