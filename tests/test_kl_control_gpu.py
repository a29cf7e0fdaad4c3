"""PPO KL control on the GPU: stage 1's diagnostics against f64 torch, the controller in clip + Adam against numpy f32 on hand-filled
sums, the controller switched off against the plain step, GraphedPPO against the eager update on recipe R (tests/kl_util.py), and a
short real run.  Every random input is drawn on the CPU and copied to the device."""
import copy
import os
import types

import numpy as np
import pytest
import torch

from solorl_amd.ppo.kl_control import kl_rule

from . import kl_util as R

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _policy(dev, O, OC, A, seed):
    from solorl_amd.ppo import Policy
    from solorl_amd.vec_env import Box
    torch.manual_seed(seed)
    pol = Policy((O,), Box(-np.ones(A), np.ones(A)), None, {"hidden_size": 64}, **({} if OC is None else {"critic_obs_dim": OC}))
    with torch.no_grad():
        pol.pi_dist.logstd.normal_(0, 0.3)
        for p in pol.parameters():
            if p.dim() == 1 and p is not pol.pi_dist.logstd:
                p.normal_(0, 0.1)
    return pol.to(dev)


# ---------------------------------------------------------------------------------------------------------------- 1. stage 1
@pytest.mark.parametrize("T,N,m,offset", [(4, 32, 64, 0), (16, 128, 1024, 512)])
@pytest.mark.parametrize("O,OC,A,family", [(76, None, 12, "templated"), (30, None, 8, "templated"), (38, 58, 12, "templated"),
                                           (79, None, 12, "generic"), (79, 96, 12, "generic")])
def test_stage1_diagnostics_match_f64_and_leave_every_other_output_alone(gpu_device, O, OC, A, family, T, N, m, offset):
    from solorl_amd.ppo import RolloutStorage
    from solorl_amd.ppo import dist as D
    from solorl_amd.ppo.fused import MiniBatchGrad
    dev, clip, n = gpu_device, 0.1, T * N
    pol = _policy(dev, O, OC, A, seed=1)
    g = torch.Generator().manual_seed(2)
    st = RolloutStorage(T, N, (O,), A, dev, critic_obs_dim=OC)
    for t in (st.obs, st.actions, st.value_preds, st.returns) + (() if OC is None else (st.critic_obs,)):
        t.copy_(torch.randn(t.shape, generator=g))
    flat = lambda x: x.reshape(n, *x.shape[2:])
    with torch.no_grad():
        _, lp, _ = pol.evaluate_actions(flat(st.obs[:-1]), flat(st.actions), **({} if OC is None else {"critic_inputs": flat(st.critic_obs[:-1])}))
        noise = 0.15 * torch.randn(lp.shape, generator=g).to(dev)
        for b in (1.0 - clip, 1.0 + clip):                                  # every ratio 1e-3 away from 1 +- clip: arithmetic, not tie-breaking
            noise = torch.where((torch.exp(-noise) - b).abs() < 1e-3, noise + 0.01, noise)
        st.action_log_probs.copy_((lp + noise).view(T, N, 1))
    adv = torch.randn(n, 1, generator=g).to(dev)
    perm = torch.randperm(n, generator=g).to(dev)
    off = torch.full((), offset, dtype=torch.long, device=dev)
    bucket = D.FlatGradBucket(pol.parameters())
    outs = []
    for diagnostics in (False, True):
        mb = MiniBatchGrad(pol, st, m, clip, 0.5, 0.01, True, perm, off, adv, family=family, diagnostics=diagnostics)
        for t in mb.buf.values():
            t.fill_(-7.0)
        bucket.flat.fill_(123.0)
        mb()
        torch.cuda.synchronize()
        outs.append(dict({k: t.clone() for k, t in mb.buf.items()}, psum=mb.psum.clone(), ent=mb.ent.clone(), grad=bucket.flat.clone(),
                         **({} if OC is None else {"cxt0": mb.cxt0.clone()})))
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k                        # the bits of the plain entry points
    assert mb.diag.shape == (m // 32, 2)
    # f64 torch on the same rows
    idx = perm[offset:offset + m]
    p64 = copy.deepcopy(pol).double()
    with torch.no_grad():
        _, lp64, _ = p64.evaluate_actions(flat(st.obs[:-1])[idx].double(), flat(st.actions)[idx].double(),
                                          **({} if OC is None else {"critic_inputs": flat(st.critic_obs[:-1])[idx].double()}))
        d = lp64 - flat(st.action_log_probs)[idx].double()
        r = torch.exp(d)
    assert ((r - (1 - clip)).abs().min() > 5e-4) and ((r - (1 + clip)).abs().min() > 5e-4)
    kl_ref, count = float(((r - 1.0) - d).mean()), int(((r < 1 - clip) | (r > 1 + clip)).sum())
    sums = mb.diag.double().sum(0).tolist()
    print("kl", sums[0] / m, "f64", kl_ref, "clipped", sums[1], "of", m)
    assert count > 0 and sums[1] == float(count)                             # the clip fraction is exactly count / m
    assert abs(sums[0] / m - kl_ref) <= R.bound(kl_ref)
    # per tile too: tile i holds rows 32 i .. 32 i + 31 of the mini-batch
    tiles = ((r < 1 - clip) | (r > 1 + clip)).double().reshape(m // 32, 32).sum(1)
    assert torch.equal(mb.diag[:, 1].double().cpu(), tiles.cpu())


# ---------------------------------------------------------------------------------------------------------------- 2. the controller
def _wave_sum(x):
    """wave_sum of csrc/solorl_ppo.hip on [waves][64] f32: the xor butterfly"""
    lane = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        x = (x + x[:, lane ^ s]).astype(F)
    return x


def _reduce_diag(diag):
    """the kernel's fixed order: thread t adds rows t, t + 1024, ...; then the wavefront; then the 16 wavefront sums in order"""
    nw = diag.shape[0]
    out = []
    for c in range(2):
        acc = np.zeros(1024, F)
        for r0 in range(0, nw, 1024):
            rows = diag[r0:r0 + 1024, c]
            acc[:len(rows)] = (acc[:len(rows)] + rows).astype(F)
        w = _wave_sum(acc.reshape(16, 64))[:, 0]
        t = F(0)
        for v in w:
            t = F(t + v)
        out.append(t)
    return out


def _same(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a) & np.isnan(b)                                           # (a NaN's payload is the hardware's business)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | nan))


def _controller(dev, m, kl_control, pol=None, lr=1e-3):
    from solorl_amd.ppo import RolloutStorage
    from solorl_amd.ppo import dist as D
    from solorl_amd.ppo.fused import ClipAdam, MiniBatchGrad
    pol = _policy(dev, 76, None, 12, seed=9) if pol is None else pol
    st = RolloutStorage(4, 64, (76,), 12, dev)                               # (stage 1 is never run here: only its pointers are taken)
    bucket = D.FlatGradBucket(pol.parameters())
    off = torch.zeros((), dtype=torch.long, device=dev)
    mb = MiniBatchGrad(pol, st, m, 0.1, 0.5, 0.01, True, torch.arange(256, device=dev), off, torch.zeros(256, 1, device=dev), diagnostics=True)
    lr_t = torch.tensor(lr, device=dev)
    ca = ClipAdam(mb, lr_t, 0.5, offset=off, offset_increment=m, kl_control=kl_control)
    return pol, bucket, mb, ca, lr_t, off


# per step: the KL the sums are scaled to (None: as drawn), or a value planted in one row
STEPS = [("scale", 0.05), ("scale", 0.001), ("scale", 0.01), ("scale", 0.05), ("scale", 0.0), ("scale", -1e-4), ("plant", float("nan")),
         ("plant", float("inf")), ("scale", 0.001), ("scale", 0.3)]


@pytest.mark.parametrize("m", [64, 32768, 81920])        # 2, 1024 and 2560 rows of diag: idle threads, one row each, two or three rows each
@pytest.mark.parametrize("desired,target,lr0,bounds", [(0.01, None, 1e-3, (1e-5, 1e-2)), (0.01, None, 1.2e-5, (1e-5, 1.5e-5)), (None, None, 1e-3, (1e-5, 1e-2)),
                                                       (0.01, 0.1, 1e-3, (1e-5, 1e-2))])
def test_controller_matches_numpy_f32(gpu_device, m, desired, target, lr0, bounds):
    dev = gpu_device
    cap = len(STEPS) - 2                                                     # (the last two steps fall off the log)
    _pol, bucket, mb, ca, lr_t, off = _controller(dev, m, dict(desired_kl=desired, target_kl=target, lr_bounds=bounds, log_capacity=cap), lr=lr0)
    rng = np.random.default_rng(m)
    g = torch.Generator().manual_seed(3)
    lr, stopped, state, log = F(lr0), False, np.zeros(8, F), np.zeros((cap, 4), F)
    for i, (how, val) in enumerate(STEPS):
        diag = np.stack([rng.uniform(0.0, 2.0, m // 32), rng.integers(0, 33, m // 32)], 1).astype(F)
        if how == "scale":
            diag[:, 0] *= F(val * m / max(float(diag[:, 0].astype(np.float64).sum()), 1e-30))
        else:
            diag[(7 * i) % (m // 32), 0] = val
        mb.diag.copy_(torch.from_numpy(diag))
        bucket.flat.copy_(torch.randn(bucket.flat.shape, generator=g))
        ca()
        s0, s1 = _reduce_diag(diag)
        kl, cf = F(s0 / F(m)), F(s1 / F(m))
        lr, stopped = kl_rule(kl, lr, stopped, desired, target, 1.5, bounds[0], bounds[1])
        applied = F(0.0 if stopped else 1.0)
        if i < cap:
            log[i] = (kl, cf, lr, applied)
        state[:4] = (state[0] + F(1), state[1] + applied, state[2] + kl, state[3] + cf)
        state[4:] = (F(stopped), kl, cf, lr)
        assert _same(ca.kl_state.cpu().numpy(), state), (i, ca.kl_state.tolist(), state.tolist())
        assert _same(lr_t.item(), lr), (i, lr_t.item(), lr)
    assert _same(ca.kl_log.cpu().numpy(), log)
    assert off.item() == len(STEPS) * m and ca.step.item() == float(state[1])
    d = ca.kl_diagnostics()
    assert d["steps"] == len(STEPS) and d["steps_applied"] == int(state[1]) and d["stopped"] is bool(stopped)
    if target:
        assert stopped and state[1] == 9.0                                   # the 0.3 of the last step is above 1.5 x 0.1
    ca.clear_kl()
    assert ca.kl_state.abs().sum().item() == 0.0 and ca.kl_log.abs().sum().item() == 0.0


def test_a_stop_at_step_2_of_5_leaves_a_2_step_run(gpu_device):
    dev, m = gpu_device, 1024
    pol_a, bucket_a, mb_a, ca_a, _lr_a, off_a = _controller(dev, m, dict(target_kl=0.01, log_capacity=5))
    pol_b, bucket_b, _mb_b, ca_b, _lr_b, _off_b = _controller(dev, m, dict(target_kl=0.01, log_capacity=5), pol=copy.deepcopy(pol_a))
    g = torch.Generator().manual_seed(4)
    grads = [torch.randn(bucket_a.flat.shape, generator=g).to(dev) for _ in range(5)]
    fill = lambda mb, kl: mb.diag.copy_(torch.tensor([kl * 32.0, 3.0], device=dev).expand(m // 32, 2))
    for i, kl in enumerate([0.002, 0.004, 0.05, 0.001, 0.0]):               # the third is above 1.5 x 0.01; what follows would not be
        fill(mb_a, kl)
        bucket_a.flat.copy_(grads[i])
        ca_a()
        if i < 2:
            fill(_mb_b, kl)
            bucket_b.flat.copy_(grads[i])
            ca_b()
    for p, q in zip(pol_a.parameters(), pol_b.parameters()):
        assert torch.equal(p, q)
    assert torch.equal(ca_a.exp_avg, ca_b.exp_avg) and torch.equal(ca_a.exp_avg_sq, ca_b.exp_avg_sq) and ca_a.step.item() == ca_b.step.item() == 2.0
    assert off_a.item() == 5 * m
    s = ca_a.kl_state.tolist()
    assert s[0] == 5.0 and s[1] == 2.0 and s[4] == 1.0
    assert ca_a.kl_log[:, 3].tolist() == [1.0, 1.0, 0.0, 0.0, 0.0]
    assert ca_a.kl_diagnostics()["stopped"] is True and ca_b.kl_diagnostics()["stopped"] is False


# ---------------------------------------------------------------------------------------------------------------- 3. control off
@pytest.mark.parametrize("O,OC,A,family", [(76, None, 12, "templated"), (38, 58, 12, "templated"), (79, None, 12, "generic")])
def test_with_control_off_the_step_is_the_plain_one_bit_for_bit(gpu_device, O, OC, A, family):
    from solorl_amd.ppo import RolloutStorage
    from solorl_amd.ppo import dist as D
    from solorl_amd.ppo.fused import ClipAdam, MiniBatchGrad
    dev, m = gpu_device, 64
    pol_a = _policy(dev, O, OC, A, seed=9)
    pol_b = copy.deepcopy(pol_a)
    runs = []
    for pol, kl_control in ((pol_a, None), (pol_b, {})):
        st = RolloutStorage(4, 64, (O,), A, dev, critic_obs_dim=OC)
        bucket = D.FlatGradBucket(pol.parameters())
        off = torch.zeros((), dtype=torch.long, device=dev)
        mb = MiniBatchGrad(pol, st, m, 0.1, 0.5, 0.01, True, torch.arange(256, device=dev), off, torch.zeros(256, 1, device=dev), family=family,
                           diagnostics=kl_control is not None)
        if kl_control is not None:
            mb.diag.copy_(torch.tensor([[40.0, 5.0], [0.3, 1.0]]))           # a KL of 0.63: nothing may act on it
        ca = ClipAdam(mb, torch.tensor(1e-3, device=dev), None, weight_decay=1e-3, offset=off, offset_increment=m, kl_control=kl_control)
        runs.append((bucket, ca, off))
    g = torch.Generator().manual_seed(1)
    for it in range(3):
        flat = (torch.randn(runs[0][0].flat.shape, generator=g) * (3.0 if it % 2 else 0.01)).to(dev)
        for bucket, ca, _off in runs:
            bucket.flat.copy_(flat)
            ca()
    for p, q in zip(pol_a.parameters(), pol_b.parameters()):
        assert torch.equal(p, q)
    (_, ca_a, off_a), (_, ca_b, off_b) = runs
    assert torch.equal(ca_a.exp_avg, ca_b.exp_avg) and torch.equal(ca_a.exp_avg_sq, ca_b.exp_avg_sq)
    assert ca_a.step.item() == ca_b.step.item() == 3.0 and off_a.item() == off_b.item() == 3 * m and ca_b.lr.item() == ca_a.lr.item()
    s = ca_b.kl_state.tolist()
    assert s[0] == 3.0 and s[1] == 3.0 and s[4] == 0.0 and abs(s[5] - 40.3 / 64) < 1e-6 and s[6] == 6.0 / 64


# ---------------------------------------------------------------------------------------------------------------- 4. end to end on R
class _Snapshots:
    """stands in for a captured graph: the parameters in front of every replay"""

    def __init__(self, graph, policy):
        self.graph, self.policy, self.snaps = graph, policy, []

    def replay(self):
        self.snaps.append(R.snapshot(self.policy))
        self.graph.replay()


def _eager_cpu(O=76, **kw):
    from solorl_amd.ppo.ppo import PPO
    pol = R.recipe_policy(O)
    st = R.recipe_storage(pol)
    agent = PPO(pol, *R.PPO_ARGS, **R.PPO_KW, **kw)
    snaps = []
    agent.optimizer.register_step_pre_hook(lambda *_a: snaps.append(R.snapshot(pol)))
    agent.update(st)
    return agent, pol, st, snaps


def _graphed(dev, O=76, **kw):
    from solorl_amd.ppo.graphs import GraphedPPO
    pol = R.recipe_policy(O)
    st_cpu = R.recipe_storage(pol)
    pol = pol.to(dev)
    st = R.storage_to(st_cpu, dev)
    agent = GraphedPPO(pol, *R.PPO_ARGS, **R.PPO_KW, **kw)
    agent._build(st)
    agent._g1 = _Snapshots(agent._g1, pol)
    agent.update(st)
    return agent, pol, st, st_cpu


def _compare_with_eager(agent, pol, st_cpu, eager, pol_e, snaps_e, desired=None, target=None):
    log, log_e = agent.last_step_log.numpy(), eager.last_step_log.numpy()
    snaps = agent._g1.snaps
    kls = [R.kl64(pol, s, st_cpu) for s in snaps]
    kls_e = [R.kl64(pol_e, s, st_cpu) for s in snaps_e] + ([R.kl64(pol_e, R.snapshot(pol_e), st_cpu)] if target else [])
    print("KL per step: kernels", log[:, 0].tolist(), "\n f64 of their parameters", kls, "\n eager", log_e[:, 0].tolist(), "\n f64", kls_e)
    R.assert_margins(kls, desired, target)
    R.assert_margins(kls_e, desired, target)
    assert len(log) == len(log_e) == len(kls)
    assert [int(R.f32_bits(x)) for x in log[:, 2]] == [int(R.f32_bits(x)) for x in log_e[:, 2]]         # the lr bits at every step
    assert log[:, 3].tolist() == log_e[:, 3].tolist()                                                    # ... and the applied flags
    n = st_cpu.num_samples
    for i, (row, k, s) in enumerate(zip(log, kls, snaps)):
        assert abs(float(row[0]) - k) <= R.bound(k), (i, row[0], k)
        r = R.ratios64(pol, s, st_cpu)
        cf = float(((r < 1 - R.CLIP) | (r > 1 + R.CLIP)).double().mean())
        near = int((((r - (1 - R.CLIP)).abs() < 1e-4) | ((r - (1 + R.CLIP)).abs() < 1e-4)).sum())
        assert abs(float(row[1]) - cf) <= near / n + 1e-9, (i, row[1], cf, near)
    va = torch.cat([p.detach().flatten().cpu() for p in pol.parameters()])
    vb = torch.cat([p.detach().flatten() for p in pol_e.parameters()])
    assert ((va - vb).norm() / vb.norm()).item() < 1e-3 and (va - vb).abs().max().item() < 5e-3


def test_graphed_ppo_adapts_like_eager_on_recipe_R(gpu_device):
    eager, pol_e, st_cpu, snaps_e = _eager_cpu(desired_kl=0.01)
    agent, pol, st, _ = _graphed(gpu_device, desired_kl=0.01)
    assert agent._mb is not None and agent._mb.diag is not None
    _compare_with_eager(agent, pol, st_cpu, eager, pol_e, snaps_e, desired=0.01)
    d = agent.last_diagnostics
    assert d["steps"] == d["steps_applied"] == 8 and d["stopped"] is False and abs(d["lr"] - 8.7792e-05) < 1e-8
    assert d["approx_kl"] == pytest.approx(float(agent.last_step_log[:, 0].double().mean()), rel=1e-5)
    # a second update starts from a cleared state, at the rate the first left
    lr1 = agent.last_step_log[-1, 2].item()
    agent.update(st)
    d2, log2 = agent.last_diagnostics, agent.last_step_log.numpy()
    assert d2["steps"] == 8 and log2.shape == (8, 4)
    lr, stopped = F(lr1), False
    for row in log2:
        lr, stopped = kl_rule(row[0], lr, stopped, 0.01)
        assert R.f32_bits(lr) == R.f32_bits(row[2])


def test_graphed_ppo_stops_like_eager_on_recipe_R(gpu_device):
    eager, pol_e, st_cpu, snaps_e = _eager_cpu(target_kl=0.01)
    agent, pol, st, _ = _graphed(gpu_device, target_kl=0.01)
    assert agent._mb is not None
    _compare_with_eager(agent, pol, st_cpu, eager, pol_e, snaps_e, target=0.01)
    d = agent.last_diagnostics
    assert d["steps"] == 2 and d["steps_applied"] == 1 and d["stopped"] is True
    assert agent._ca.step.item() == 1.0
    # the next update counts from zero, and its flag was cleared: from where the policy now stands the first step already reads a KL
    # beyond the threshold (step 1's of the run above), so it is this update's own stop
    agent.update(st)
    d2 = agent.last_diagnostics
    assert d2["steps"] == 1 and d2["steps_applied"] == 0 and d2["stopped"] is True and agent._ca.step.item() == 1.0
    assert abs(agent.last_step_log[0, 0].item() - eager.last_step_log[1, 0].item()) < 1e-3


def test_autograd_graph_path_adapts_like_eager_and_refuses_target_kl(gpu_device, monkeypatch):
    monkeypatch.delenv("SOLORL_POLICY_GENERIC", raising=False)              # width 79 is built by no per-shape kernel
    eager, pol_e, st_cpu, snaps_e = _eager_cpu(79, desired_kl=0.01)
    agent, pol, st, _ = _graphed(gpu_device, 79, desired_kl=0.01)
    assert agent._mb is None and agent._ca is None
    log, log_e = agent.last_step_log.numpy(), eager.last_step_log.numpy()
    kls = [R.kl64(pol, s, st_cpu) for s in agent._g1.snaps]
    print("KL per step: autograd graph", log[:, 0].tolist(), "\n f64 of its parameters", kls, "\n eager", log_e[:, 0].tolist())
    R.assert_margins(kls, 0.01)
    R.assert_margins([R.kl64(pol_e, s, st_cpu) for s in snaps_e], 0.01)
    assert [int(R.f32_bits(x)) for x in log[:, 2]] == [int(R.f32_bits(x)) for x in log_e[:, 2]] and log[:, 3].tolist() == log_e[:, 3].tolist()
    for row, k in zip(log, kls):
        assert abs(float(row[0]) - k) <= R.bound(k)
    assert agent.last_diagnostics["steps"] == 8 and R.f32_bits(agent.optimizer.param_groups[0]["lr"].item()) == R.f32_bits(log[-1, 2])
    from solorl_amd.ppo.graphs import GraphedPPO
    pol2 = R.recipe_policy(79)
    st2 = R.storage_to(R.recipe_storage(pol2), gpu_device)
    with pytest.raises(NotImplementedError, match="--generic-policy-kernels.*--no-hip-graphs"):
        GraphedPPO(pol2.to(gpu_device), *R.PPO_ARGS, **R.PPO_KW, target_kl=0.01).update(st2)


# ---------------------------------------------------------------------------------------------------------------- 5. a short real run
def _train(tmp_path, **flags):
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo.train import train
    config = load_yaml(os.path.join(ROOT, "configs", "basic12.yaml"))
    config["task"] = "walk"
    args = types.SimpleNamespace(
        num_agents=256, hidden_size=64, cuda=True, gamma=0.99, tau=0.95, clip_param=0.1, ppo_epoch=2, mini_batch_size=1024,
        lr=1e-3, l2_coef=0.0, value_loss_coef=0.5, entropy_coef=0.01, max_grad_norm=0.5, use_linear_lr_decay=False,
        use_gae=True, num_env_steps=256 * 16 * 2, seed=1, curriculum_schedule=0, log_interval=1, logdir=str(tmp_path),
        base_checkpoint=None, save_interval=10, num_steps=16, **flags)
    return train(args, config)


NEW_KEYS = ("approx_kl", "clip_fraction", "lr", "kl_stopped_steps")


def test_short_real_run_logs_the_diagnostics_only_when_asked(gpu_device, tmp_path):
    import math
    _pol, hist = _train(tmp_path, desired_kl=0.01, ppo_diagnostics=True)
    assert len(hist) == 2
    for h in hist:
        print({k: h[k] for k in NEW_KEYS})
        assert math.isfinite(h["approx_kl"]) and h["approx_kl"] >= -1e-6
        assert 0.0 <= h["clip_fraction"] <= 1.0 and 1e-5 <= h["lr"] <= 1e-2 and h["kl_stopped_steps"] == 0
    _pol, hist = _train(tmp_path)
    assert len(hist) == 2 and not any(k in h for h in hist for k in NEW_KEYS)
