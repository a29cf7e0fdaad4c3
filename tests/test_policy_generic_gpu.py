"""The width-generic policy kernels (csrc/solorl_ppo.hip: policy_act_w_kernel, ppo_grad_stage1_w_kernel, stage 2's four-input-tile case,
ppo_clip_adam_w_kernel behind the _w entry points).

1. At shapes the per-shape family builds, BITWISE against it: the order of every sum is the same by construction (layer 0 contracts
   q = 0 .. ceil(O / 8) - 1, t = 0 .. 3 into the two unit tiles in both), so there is no tolerance -- a difference means the order changed.
2. At shapes it does not build, against PyTorch, at the bounds the project already uses for its built shapes (named where they are used).
3. Through GraphedPPO / GraphedRollout with the switch SOLORL_POLICY_GENERIC.
Smallest first."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BUILT = [(76, 76, 12), (41, 41, 12), (33, 50, 8), (76, 96, 12)]
# (79, 79, 12) odd width, word path; (97, 97, 12) last group of 8 inputs half empty, four input tiles in stage 2; (84, 104, 12) float4 path
# above 96, critic wider than actor; (63, 80, 8) A = 8; (128, 128, 12) the cap
UNBUILT = [(79, 79, 12), (97, 97, 12), (84, 104, 12), (63, 80, 8), (128, 128, 12)]
T, N, M, OFFSET = 16, 128, 1024, 512          # the data of _check_minibatch_grad (tests/test_train_gpu.py): 16 x 128 rows, 1024 at offset 512
CLIP, VC, EC = 0.1, 0.5, 0.01


def _random_policy(O, OC, A, seed=0):
    """OC == O: the symmetric policy"""
    from solorl_amd.ppo import Policy
    from solorl_amd.vec_env import Box
    torch.manual_seed(seed)
    pol = Policy((O,), Box(-np.ones(A), np.ones(A)), None, {"hidden_size": 64}, critic_obs_dim=None if OC == O else OC).to(DEV)
    with torch.no_grad():
        pol.pi_dist.logstd.normal_(0, 0.3)
        for p in pol.parameters():
            if p.dim() == 1 and p is not pol.pi_dist.logstd:
                p.normal_(0, 0.1)                   # non-zero biases
    return pol


def _critic(asym, rows):
    return {"critic_inputs": rows} if asym else {}


def _storage(pol, O, OC, A, clip=CLIP):
    """the rollout rows of _check_minibatch_grad: old log-probs near the current ones, every ratio 1e-3 away from the clip boundaries"""
    from solorl_amd.ppo import RolloutStorage
    asym = OC != O
    st = RolloutStorage(T, N, (O,), A, DEV, **({"critic_obs_dim": OC} if asym else {}))
    torch.manual_seed(2)
    st.obs.normal_(); st.actions.normal_(); st.value_preds.normal_(); st.returns.normal_()
    if asym:
        st.critic_obs.normal_()
    n = T * N
    flat = lambda x: x.reshape(n, *x.shape[2:])
    with torch.no_grad():
        _, lp, _ = pol.evaluate_actions(flat(st.obs[:-1]), flat(st.actions), **_critic(asym, flat(st.critic_obs[:-1]) if asym else None))
        noise = 0.15 * torch.randn_like(lp)
        for b in (1.0 - clip, 1.0 + clip):
            near = (torch.exp(-noise) - b).abs() < 1e-3
            noise = torch.where(near, noise + 0.01, noise)
        st.action_log_probs.copy_((lp + noise).view(T, N, 1))
    adv = torch.randn(n, 1, device=DEV)
    perm = torch.randperm(n, device=DEV)
    return st, adv, perm


def _minibatch(pol, st, adv, perm, family, clipped=True):
    from solorl_amd.ppo import dist as D
    from solorl_amd.ppo.fused import MiniBatchGrad
    off = torch.full((), OFFSET, dtype=torch.long, device=DEV)
    bucket = D.FlatGradBucket(pol.parameters())
    mb = MiniBatchGrad(pol, st, M, CLIP, VC, EC, clipped, perm, off, adv, family=family)
    bucket.flat.fill_(123.0)                    # every gradient element must be overwritten
    return bucket, mb


# ------------------------------------------------------------------------------------------------ 1. bitwise at built shapes
@pytest.mark.parametrize("O,OC,A", BUILT)
def test_act_writes_the_bits_of_the_per_shape_kernels(gpu_device, O, OC, A):
    """solorl_policy_act_w against solorl_policy_act[_critic]: fewer rows than a tile, a ragged last tile; with noise and deterministic"""
    from solorl_amd.ppo.fused import GENERIC, TEMPLATED, policy_act, policy_kernel_family, policy_params
    pol = _random_policy(O, OC, A)
    assert policy_kernel_family(pol, 0) == TEMPLATED and policy_kernel_family(pol, 1) == TEMPLATED and policy_kernel_family(pol, 2) == GENERIC
    Pt, Pg = policy_params(pol, TEMPLATED), policy_params(pol, GENERIC)
    for n in (31, 1000):
        obs = torch.randn(n, O, device=DEV)
        cobs = torch.randn(n, OC, device=DEV) if OC != O else None
        for noise in (torch.randn(n, A, device=DEV), None):
            out = []
            for P in (Pt, Pg):
                v, a, l = torch.full((n, 1), 7.0, device=DEV), torch.full((n, A), 7.0, device=DEV), torch.full((n, 1), 7.0, device=DEV)
                policy_act(P, obs, noise, v, a, l, critic_obs=cobs)
                out.append((v, a, l))
            for x, y in zip(*out):
                assert torch.equal(x, y) and not bool((y == 7.0).all()), (n, (x - y).abs().max().item())


@pytest.mark.parametrize("O,OC,A", BUILT)
def test_minibatch_step_writes_the_bits_of_the_per_shape_kernels(gpu_device, O, OC, A):
    """stage 1, stage 2 + 3 and two clip + Adam steps from equal states: every work array, the gradient bucket, the loss sums, every
    parameter and both moments"""
    from solorl_amd.ppo.fused import GENERIC, TEMPLATED, ClipAdam
    pol_t = _random_policy(O, OC, A, seed=1)
    pol_g = copy.deepcopy(pol_t)
    st, adv, perm = _storage(pol_t, O, OC, A)
    sides = []
    for pol, family in ((pol_t, TEMPLATED), (pol_g, GENERIC)):
        bucket, mb = _minibatch(pol, st, adv, perm, family)
        assert mb.P.family == family
        ca = ClipAdam(mb, torch.tensor(1e-3, device=DEV), 0.5)
        mb()
        first = {k: v.clone() for k, v in mb.buf.items()}
        first["cxt0"] = None if mb.cxt0 is None else mb.cxt0.clone()
        first["bucket"], first["loss_sums"], first["logstd_sum"] = bucket.flat.clone(), mb.psum.clone(), mb.ent.clone()
        ca()
        mb()                                    # the second step's gradients, at the parameters the first one left
        ca()
        torch.cuda.synchronize()
        sides.append((first, bucket.flat.clone(), [p.detach().clone() for p in pol.parameters()], ca.exp_avg.clone(), ca.exp_avg_sq.clone(), ca.step.item()))
    (ft, gt, pt, mt, vt, stt), (fg, gg, pg, mg, vg, stg) = sides
    assert not bool((ft["bucket"] == 123.0).any())
    for k in ft:
        assert (ft[k] is None and fg[k] is None) or torch.equal(ft[k], fg[k]), k
    assert torch.equal(gt, gg) and torch.equal(mt, mg) and torch.equal(vt, vg) and stt == stg == 2.0
    assert all(torch.equal(a, b) for a, b in zip(pt, pg))
    assert not torch.equal(pt[0], next(_random_policy(O, OC, A, seed=1).parameters()))          # (the steps moved the parameters)


# ------------------------------------------------------------------------------------------------ 2. unbuilt shapes against PyTorch
@pytest.mark.parametrize("O,OC,A", UNBUILT)
def test_act_matches_torch_at_unbuilt_shapes(gpu_device, O, OC, A):
    """solorl_policy_act_w == Policy.act_into on 1000 rows (ragged), with noise and deterministic: the bounds of
    test_policy_act_kernel_matches_torch (tests/test_train_gpu.py)"""
    from solorl_amd.ppo.fused import GENERIC, policy_act, policy_kernel_family, policy_kernels_generic_supported, policy_kernels_supported, policy_params
    pol = _random_policy(O, OC, A)
    asym = OC != O
    assert policy_kernels_generic_supported(pol) and not policy_kernels_supported(pol)
    assert policy_kernel_family(pol, 0) is None and policy_kernel_family(pol, 1) == GENERIC
    P = policy_params(pol, GENERIC)
    n = 1000
    obs = torch.randn(n, O, device=DEV)
    cobs = torch.randn(n, OC, device=DEV) if asym else None
    for noise in (torch.randn(n, A, device=DEV), None):
        v0, a0, l0 = torch.empty(n, 1, device=DEV), torch.empty(n, A, device=DEV), torch.empty(n, 1, device=DEV)
        pol.act_into(obs, v0, a0, l0, noise=noise if noise is not None else torch.zeros(n, A, device=DEV), **_critic(asym, cobs))
        v1, a1, l1 = torch.full((n, 1), 7.0, device=DEV), torch.full((n, A), 7.0, device=DEV), torch.full((n, 1), 7.0, device=DEV)
        policy_act(P, obs, noise, v1, a1, l1, critic_obs=cobs)
        assert torch.allclose(v0, v1, rtol=1e-4, atol=1e-5), (v0 - v1).abs().max().item()
        assert torch.allclose(a0, a1, rtol=1e-4, atol=1e-5), (a0 - a1).abs().max().item()
        assert torch.allclose(l0, l1, rtol=1e-4, atol=1e-4), (l0 - l1).abs().max().item()


@pytest.mark.parametrize("O,OC,A", UNBUILT)
def test_minibatch_grad_matches_autograd_at_unbuilt_shapes(gpu_device, O, OC, A):
    """MiniBatchGrad on the _w stages against loss.backward() of the reference's formulas: the bounds of _check_minibatch_grad
    (tests/test_train_gpu.py; its small-batch branch: rtol 2e-3, atol 2e-5 x the largest gradient, and its loss bounds), and the gathered
    rows in xt0 / the critic's xt0 as test_minibatch_grad_kernels_match_autograd (tests/test_critic_policy_gpu.py) reads them"""
    from solorl_amd.ppo.fused import GENERIC
    asym = OC != O
    clipped = O != 97                           # (one shape on the unclipped value loss)
    pol = _random_policy(O, OC, A, seed=1)
    st, adv, perm = _storage(pol, O, OC, A)
    bucket, mb = _minibatch(pol, st, adv, perm, GENERIC, clipped)
    mb()
    g_kernel = bucket.flat.clone()
    assert not bool((g_kernel == 123.0).any())
    vl_k, al_k, ent_k = mb.losses(1)
    n = T * N
    flat = lambda x: x.reshape(n, *x.shape[2:])
    idx = perm[OFFSET:OFFSET + M]
    obs_b, act_b = flat(st.obs[:-1])[idx], flat(st.actions)[idx]
    cobs_b = flat(st.critic_obs[:-1])[idx] if asym else None
    vpred_b, ret_b, old_b, adv_b = flat(st.value_preds[:-1])[idx], flat(st.returns[:-1])[idx], flat(st.action_log_probs)[idx], adv[idx]
    values, logp, entropy = pol.evaluate_actions(obs_b, act_b, **_critic(asym, cobs_b))
    ratio = torch.exp(logp - old_b)
    al = -torch.min(ratio * adv_b, torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * adv_b).mean()
    if clipped:
        v_clipped = vpred_b + (values - vpred_b).clamp(-CLIP, CLIP)
        vl = 0.5 * torch.max((values - ret_b).pow(2), (v_clipped - ret_b).pow(2)).mean()
    else:
        vl = 0.5 * (ret_b - values).pow(2).mean()
    bucket.zero()
    (vl * VC + al - entropy * EC).backward()
    g_ref = bucket.flat
    assert (ratio < 1 - CLIP).any() and (ratio > 1 + CLIP).any()
    scale = g_ref.abs().max().item()
    print("max |gradient difference| %.3g (largest gradient %.3g)" % ((g_kernel - g_ref).abs().max().item(), scale))
    assert torch.allclose(g_kernel, g_ref, rtol=2e-3, atol=2e-5 * scale), ((g_kernel - g_ref).abs().max().item(), scale)
    assert abs(vl_k - vl.item()) < 1e-4 * max(1.0, abs(vl.item())) and abs(al_k - al.item()) < 1e-5 + 1e-4 * abs(al.item())
    assert abs(ent_k - entropy.item()) < 1e-5
    xt0 = mb.buf["xt0"].reshape(M // 32, O, 32).permute(0, 2, 1).reshape(M, O)
    assert torch.equal(xt0, obs_b)
    if asym:
        assert torch.equal(mb.cxt0.reshape(M // 32, OC, 32).permute(0, 2, 1).reshape(M, OC), cobs_b)


@pytest.mark.parametrize("O,OC,A", UNBUILT)
def test_clip_adam_matches_torch_at_unbuilt_shapes(gpu_device, O, OC, A):
    """solorl_ppo_clip_adam_w == clip_grad_norm_ + torch.optim.Adam.step over five steps, a learning rate changed in between, weight decay,
    the cursor: the bounds of test_clip_adam_kernel_on_both_widths_matches_torch (tests/test_critic_policy_gpu.py)"""
    from solorl_amd.ppo import RolloutStorage
    from solorl_amd.ppo import dist as D
    from solorl_amd.ppo.fused import GENERIC, ClipAdam, MiniBatchGrad
    asym = OC != O
    for wd, max_norm in ((0.0, 0.5), (1e-3, None)):
        pol_a = _random_policy(O, OC, A, seed=9)
        pol_b = copy.deepcopy(pol_a)
        st = RolloutStorage(4, 64, (O,), A, DEV, **({"critic_obs_dim": OC} if asym else {}))
        bucket = D.FlatGradBucket(pol_a.parameters())
        off = torch.zeros((), dtype=torch.long, device=DEV)
        mb = MiniBatchGrad(pol_a, st, 64, 0.1, 0.5, 0.01, True, torch.arange(256, device=DEV), off, torch.zeros(256, 1, device=DEV), family=GENERIC)
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


# ------------------------------------------------------------------------------------------------ 3. through the graphs
def _update_storage(O, OC, A, T_=16, N_=64):
    from solorl_amd.ppo import RolloutStorage
    torch.manual_seed(0)
    st = RolloutStorage(T_, N_, (O,), A, DEV, **({"critic_obs_dim": OC} if OC != O else {}))
    st.obs.normal_(); st.actions.normal_(); st.rewards.normal_(); st.value_preds.normal_()
    if OC != O:
        st.critic_obs.normal_()
    st.action_log_probs.normal_().mul_(0.1).sub_(10)
    st.masks.copy_((torch.rand_like(st.masks) > 0.05).float())
    st.compute_returns(torch.randn(N_, 1, device=DEV), True, 0.99, 0.95)
    return st


def test_graphed_update_runs_an_unbuilt_shape_on_the_kernels(gpu_device, monkeypatch):
    """(45, 62, 12), the shape test_graphed_update_of_an_asymmetric_policy_matches_eager (tests/test_critic_ppo_gpu.py) pins to autograd
    with the switch unset: with it at 1 the captured step is the kernels', and two updates match eager PPO at that test's bounds"""
    from solorl_amd.ppo import PPO
    from solorl_amd.ppo.fused import GENERIC
    from solorl_amd.ppo.graphs import GraphedPPO
    O, OC, A = 45, 62, 12
    st = _update_storage(O, OC, A)
    pol_a = _random_policy(O, OC, A, seed=4)
    pol_b = copy.deepcopy(pol_a)
    monkeypatch.delenv("SOLORL_POLICY_GENERIC", raising=False)
    assert not GraphedPPO(copy.deepcopy(pol_a), 0.1, 2, 256, 0.5, 0.01, lr=1e-3, max_grad_norm=0.5).fused_mlp
    monkeypatch.setenv("SOLORL_POLICY_GENERIC", "1")
    eager = PPO(pol_a, 0.1, 2, 256, 0.5, 0.01, lr=1e-3, max_grad_norm=0.5)
    graph = GraphedPPO(pol_b, 0.1, 2, 256, 0.5, 0.01, lr=1e-3, max_grad_norm=0.5)
    assert graph.fused_mlp
    w0 = pol_b.base.critic[0].weight.detach().clone()
    for it in range(2):                 # second round replays the graph captured in the first
        torch.manual_seed(5 + it); la = eager.update(st)
        torch.manual_seed(5 + it); lb = graph.update(st)
        assert graph._mb is not None and graph._mb.P.family == GENERIC and graph._ca is not None
        assert np.allclose(la, lb, rtol=1e-4, atol=1e-5), (la, lb)
        va = torch.cat([p.detach().flatten() for p in pol_a.parameters()])
        vb = torch.cat([p.detach().flatten() for p in pol_b.parameters()])
        assert ((va - vb).norm() / va.norm()).item() < 1e-3 and (va - vb).abs().max().item() < 5e-3
    assert bool((pol_b.base.critic[0].weight != w0)[:, O:].any())


def test_graphed_rollout_of_a_commanded_env_with_history_acts_on_the_kernels(gpu_device, monkeypatch):
    """8 steps of 8 envs, Solo12 walk with velocity commands at one history level -- 79 words, the width --commands costs 60 % at: one
    solorl_policy_act_w launch per step; the stored values and log-probs equal get_value / evaluate_actions of the stored rows at the 1e-5
    and 1e-4 of test_graphed_rollout_on_the_kernel_path (tests/test_critic_policy_gpu.py)"""
    from solorl_amd import _native
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.ppo import RolloutStorage
    from solorl_amd.ppo.fused import GENERIC
    from solorl_amd.ppo.graphs import GraphedRollout, _policy_family
    from solorl_amd.vec_env import SoloVecEnv
    N_, T_ = 8, 8
    cfg = default_config(ROBOT_SOLO12, TASK_WALK); cfg.num_history_stack = 1
    env = SoloVecEnv(cfg, N_, device=DEV, seed=3, commands={"lin_vel_x": [0.0, 1.0], "interval": [2, 4]})
    assert env.obs_dim == 79
    pol = _random_policy(79, 79, 12, seed=2)
    monkeypatch.delenv("SOLORL_POLICY_GENERIC", raising=False)
    assert _policy_family(pol) is None
    monkeypatch.setenv("SOLORL_POLICY_GENERIC", "1")
    assert _policy_family(pol) == GENERIC
    st = RolloutStorage(T_, N_, (79,), 12, DEV)
    st.obs[0].copy_(env.reset())
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
        roll = GraphedRollout(env, pol, st, T_)
        roll()
    finally:
        _native._LIB = real
    torch.cuda.synchronize()
    assert not roll.step_act and roll.windows is None and calls.count("solorl_policy_act_w") == T_
    assert "solorl_policy_act" not in calls and "solorl_step_act" not in calls
    with torch.no_grad():
        for t in range(T_):
            v = pol.get_value(st.obs[t])
            _, lp, _ = pol.evaluate_actions(st.obs[t], st.actions[t])
            assert torch.allclose(v, st.value_preds[t], atol=1e-5) and torch.allclose(lp, st.action_log_probs[t], atol=1e-4), t
    assert torch.isfinite(st.obs).all() and bool((st.obs[1:] != st.obs[:-1]).any())
    env.close()


def test_graphed_update_at_switch_2_leaves_the_bits_of_the_default_path(gpu_device, monkeypatch):
    """(76, 76, 12): one graphed update on the generic family (switch 2) leaves every parameter torch.equal to the update with the switch unset"""
    from solorl_amd.ppo.fused import GENERIC, TEMPLATED
    from solorl_amd.ppo.graphs import GraphedPPO
    O, OC, A = 76, 76, 12
    st = _update_storage(O, OC, A, 16, 128)
    pol0 = _random_policy(O, OC, A, seed=4)
    out = []
    for switch, family in ((None, TEMPLATED), ("2", GENERIC)):
        if switch is None:
            monkeypatch.delenv("SOLORL_POLICY_GENERIC", raising=False)
        else:
            monkeypatch.setenv("SOLORL_POLICY_GENERIC", switch)
        pol = copy.deepcopy(pol0)
        graph = GraphedPPO(pol, 0.1, 2, 512, 0.5, 0.01, lr=1e-3, max_grad_norm=0.5)
        torch.manual_seed(5)
        losses = graph.update(st)
        assert graph._mb is not None and graph._mb.P.family == family
        out.append((losses, [p.detach().clone() for p in pol.parameters()]))
    (la, pa), (lb, pb) = out
    assert la == lb and all(torch.equal(a, b) for a, b in zip(pa, pb))
    assert not torch.equal(pa[0], next(pol0.parameters()))
