"""Shared by the KL control tests (test_kl_control_cpu.py / test_kl_control_gpu.py): recipe R -- one policy, one rollout, one PPO
configuration, every random number drawn on the CPU -- the f64 recomputation of a step's KL estimate, and the thresholds a step's KL
must keep its distance from for a decision to be comparable between two implementations."""
import copy

import numpy as np
import torch

from solorl_amd.ppo import Policy, RolloutStorage
from solorl_amd.vec_env import Box

CLIP, EPOCHS, MINI_BATCH, LR = 0.1, 8, 1024, 1e-3
PPO_ARGS = (CLIP, EPOCHS, MINI_BATCH, 0.5, 0.01)          # clip, epochs, mini-batch (= the whole batch), value coefficient, entropy coefficient
PPO_KW = dict(lr=LR, max_grad_norm=0.5)


def recipe_policy(O=76):
    """recipe R's policy; O: another observation width (a shape the per-shape kernels are not built for)"""
    torch.manual_seed(4)
    pol = Policy((O,), Box(-np.ones(12), np.ones(12)), None, {"hidden_size": 64})
    with torch.no_grad():
        pol.pi_dist.logstd.normal_(0, 0.3)
        for p in pol.parameters():
            if p.dim() == 1 and p is not pol.pi_dist.logstd:
                p.normal_(0, 0.1)
    return pol


def recipe_storage(policy):
    g = torch.Generator().manual_seed(2)
    O = policy.base.features[0].in_features
    st = RolloutStorage(16, 64, (O,), 12, torch.device("cpu"))
    for t in (st.obs, st.actions, st.value_preds, st.returns):
        t.copy_(torch.randn(t.shape, generator=g))
    with torch.no_grad():
        _, logp, _ = policy.evaluate_actions(st.obs[:-1].reshape(-1, O), st.actions.reshape(-1, 12))
    st.action_log_probs.copy_((logp + 0.05 * torch.randn(logp.shape, generator=g)).reshape(16, 64, 1))
    return st


def storage_to(st, device):
    out = RolloutStorage(st.num_steps, st.num_agents, tuple(st.obs.shape[2:]), st.actions.shape[-1], device)
    for k in ("obs", "actions", "value_preds", "returns", "action_log_probs", "rewards", "masks"):
        getattr(out, k).copy_(getattr(st, k))
    return out


def snapshot(policy):
    return [p.detach().cpu().clone() for p in policy.parameters()]


def ratios64(policy, params, st):
    """the f64 ratios pi_new / pi_old of every sample with the f32 parameter values `params`"""
    p64 = copy.deepcopy(policy).cpu().double()
    with torch.no_grad():
        for p, v in zip(p64.parameters(), params):
            p.copy_(v.double())
        n = st.num_samples
        _, logp, _ = p64.evaluate_actions(st.obs[:-1].reshape(n, -1).cpu().double(), st.actions.reshape(n, -1).cpu().double())
        return torch.exp(logp - st.action_log_probs.reshape(n, 1).cpu().double())


def kl64(policy, params, st):
    r = ratios64(policy, params, st)
    return float(((r - 1.0) - torch.log(r)).mean())


def thresholds(desired_kl=None, target_kl=None):
    return ([2.0 * desired_kl, desired_kl / 2.0] if desired_kl else []) + ([1.5 * target_kl] if target_kl else [])


def assert_margins(kls, desired_kl=None, target_kl=None, margin=0.10):
    """every step's f64 KL lies at least 10 % from every threshold: f32 rounding cannot turn a decision"""
    for i, k in enumerate(kls):
        for th in thresholds(desired_kl, target_kl):
            assert abs(k - th) >= margin * th, "step %d: KL %g within %g %% of the threshold %g" % (i, k, 100 * margin, th)


def bound(kl):
    """the bound tests/test_train_gpu.py holds the action loss to"""
    return 1e-5 + 1e-4 * abs(kl)


def f32_bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)
