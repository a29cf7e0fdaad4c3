"""The asymmetric actor-critic in PyTorch, on the CPU: a Policy whose critic reads rows of its own width, rollout storage that carries
them, one PPO.update through both, and the launcher's flag -- and that the symmetric forms give what they gave."""
import os

import numpy as np
import pytest
import torch

from solorl_amd.ppo import Policy
from solorl_amd.ppo.ppo import PPO
from solorl_amd.ppo.storage import RolloutStorage
from solorl_amd.vec_env import Box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O, OC, A = 41, 58, 12
BOX = Box(-np.ones(A), np.ones(A))


def _policy(critic=OC, seed=0):
    torch.manual_seed(seed)
    return Policy((O,), BOX, None, {"hidden_size": 64}, critic_obs_dim=critic)


def test_symmetric_construction_is_what_it_was():
    sym = Policy((O,), BOX, None, {"hidden_size": 64})
    assert sym.critic_obs_dim is None
    shapes = {k: tuple(v.shape) for k, v in sym.state_dict().items()}
    assert shapes == {"base.features.0.weight": (64, O), "base.features.0.bias": (64,), "base.features.2.weight": (64, 64), "base.features.2.bias": (64,),
                      "base.critic.0.weight": (64, O), "base.critic.0.bias": (64,), "base.critic.2.weight": (64, 64), "base.critic.2.bias": (64,),
                      "base.critic.4.weight": (1, 64), "base.critic.4.bias": (1,), "pi_dist.mean.weight": (A, 64), "pi_dist.mean.bias": (A,),
                      "pi_dist.logstd": (A,)}
    asym = _policy()
    wide = {k: tuple(v.shape) for k, v in asym.state_dict().items()}
    assert list(wide) == list(shapes) and wide.pop("base.critic.0.weight") == (64, OC)       # the same names, one other shape
    shapes.pop("base.critic.0.weight")
    assert wide == shapes and asym.critic_obs_dim == OC
    # the actor of an asymmetric policy is initialised like the symmetric one's (the features come first)
    a, b = _policy(None, seed=3), _policy(OC, seed=3)
    assert torch.equal(a.base.features[0].weight, b.base.features[0].weight)
    x = torch.randn(5, O)
    with pytest.raises(ValueError, match="without critic_obs_dim"):
        sym.act(x, critic_inputs=torch.randn(5, OC))
    for call in (lambda: asym.act(x), lambda: asym.heads(x), lambda: asym.get_value(x), lambda: asym.evaluate_actions(x, torch.zeros(5, A)),
                 lambda: asym.act_into(x, torch.zeros(5, 1), torch.zeros(5, A), torch.zeros(5, 1))):
        with pytest.raises(ValueError, match=r"critic_inputs \[.., 58\] are required"):
            call()


def test_actor_and_critic_read_their_own_rows():
    pol = _policy()
    x, c = torch.randn(7, O), torch.randn(7, OC)
    x2, c2 = torch.randn(7, O), torch.randn(7, OC)
    act = torch.randn(7, A)
    with torch.no_grad():
        v, lp, ent = pol.evaluate_actions(x, act, critic_inputs=c)
        v_x2, lp_x2, _ = pol.evaluate_actions(x2, act, critic_inputs=c)
        v_c2, lp_c2, _ = pol.evaluate_actions(x, act, critic_inputs=c2)
        assert torch.equal(v, v_x2) and not torch.equal(lp, lp_x2)               # other actor rows: the same values
        assert torch.equal(lp, lp_c2) and not torch.equal(v, v_c2)               # other critic rows: the same log-probs
        assert torch.equal(pol.get_value(x, critic_inputs=c), v) and torch.equal(pol.get_value(None, critic_inputs=c), v)
        hv, mean, logstd = pol.heads(x, critic_inputs=c)
        assert torch.equal(hv, v)
        va, a_det, lpa = pol.act(x, deterministic=True, critic_inputs=c)
        assert torch.equal(va, v) and torch.equal(a_det, mean) and torch.equal(pol.act_actor(x, deterministic=True), mean)
        assert torch.equal(pol.act(x, deterministic=True, critic_inputs=c2)[1], a_det)
        noise = torch.randn(7, A)
        vo, ao, lo = torch.zeros(7, 1), torch.zeros(7, A), torch.zeros(7, 1)
        pol.act_into(x, vo, ao, lo, noise=noise, critic_inputs=c)
        assert torch.allclose(vo, v, rtol=0, atol=1e-6) and torch.allclose(ao, mean + torch.exp(logstd) * noise, rtol=0, atol=1e-6)
        assert torch.allclose(lo, pol.evaluate_actions(x, ao, critic_inputs=c)[1], rtol=0, atol=1e-5)
        vo2 = torch.zeros(7, 1)
        pol.act_into(x, vo2, ao, lo, noise=noise, critic_inputs=c2)
        assert not torch.equal(vo2, vo)


def _fill(st, T, N, asym, seed=5):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    st.obs[0].copy_(r(N, O))
    if asym:
        st.critic_obs[0].copy_(r(N, OC))
    for t in range(T):
        kw = {"critic_obs": r(N, OC)} if asym else {}
        st.append(r(N, O), r(N, A), r(N, 1), r(N, 1), r(N, 1), (torch.rand(N, 1, generator=g) > 0.1).float(), **kw)
    st.compute_returns(r(N, 1), True, 0.99, 0.95)


def test_storage_carries_and_gathers_the_critic_rows():
    T, N = 6, 8
    sym = RolloutStorage(T, N, (O,), A, "cpu")
    assert sym.critic_obs is None
    _fill(sym, T, N, False)
    adv = sym.returns[:-1] - sym.value_preds[:-1]
    assert all(len(b) == 7 for b in sym.batch_generator(adv, 16))                 # a symmetric storage yields the reference's seven
    with pytest.raises(ValueError, match="critic_obs goes with"):
        sym.append(sym.obs[0], sym.actions[0], sym.action_log_probs[0], sym.value_preds[0], sym.rewards[0], sym.masks[0], critic_obs=torch.zeros(N, OC))
    st = RolloutStorage(T, N, (O,), A, "cpu", critic_obs_dim=OC)
    assert tuple(st.critic_obs.shape) == (T + 1, N, OC)
    _fill(st, T, N, True)
    assert st.step == 0 and bool(st.critic_obs.ne(0).all())
    with pytest.raises(ValueError, match="critic_obs goes with"):
        st.append(st.obs[0], st.actions[0], st.action_log_probs[0], st.value_preds[0], st.rewards[0], st.masks[0])
    # every row of a batch is one (t, n) of the storage: the critic row gathered is the one stored beside the actor's row
    flat_o, flat_c = st.obs[:-1].reshape(T * N, O), st.critic_obs[:-1].reshape(T * N, OC)
    seen = 0
    for b in st.batch_generator(st.returns[:-1] - st.value_preds[:-1], 16):
        assert len(b) == 8 and tuple(b[7].shape) == (16, OC)
        for o_row, c_row in zip(b[0], b[7]):
            k = int((flat_o == o_row).all(dim=1).nonzero()[0, 0])
            assert torch.equal(flat_c[k], c_row)
        seen += 16
    assert seen == T * N
    last_o, last_c = st.obs[-1].clone(), st.critic_obs[-1].clone()
    st.reset()
    assert torch.equal(st.obs[0], last_o) and torch.equal(st.critic_obs[0], last_c)


def test_one_update_moves_the_wide_critic_layer():
    T, N = 6, 8
    pol = _policy()
    st = RolloutStorage(T, N, (O,), A, "cpu", critic_obs_dim=OC)
    _fill(st, T, N, True)
    before = {k: v.clone() for k, v in pol.state_dict().items()}
    agent = PPO(pol, 0.2, 2, 16, 0.5, 0.01, lr=1e-3, max_grad_norm=0.5)
    v, a, e = agent.update(st)
    assert all(np.isfinite(x) for x in (v, a, e))
    after = pol.state_dict()
    assert tuple(after["base.critic.0.weight"].shape) == (64, OC)
    for k in before:
        assert not torch.equal(before[k], after[k]), k
    assert bool((before["base.critic.0.weight"] != after["base.critic.0.weight"])[:, O:].any()), "the columns of the privileged words moved"
    # a symmetric policy on a symmetric storage updates as before
    sym, st2 = _policy(None), RolloutStorage(T, N, (O,), A, "cpu")
    _fill(st2, T, N, False)
    assert all(np.isfinite(x) for x in PPO(sym, 0.2, 1, 16, 0.5, 0.01, lr=1e-3, max_grad_norm=0.5).update(st2))
    # and the two do not mix
    with pytest.raises(ValueError, match="critic_inputs"):
        PPO(_policy(), 0.2, 1, 16, 0.5, 0.01, lr=1e-3).update(st2)


def test_policy_kernels_are_claimed_for_the_built_shapes_only():
    from solorl_amd.ppo import fused
    assert {s for s in fused._SUPPORTED if s[1] != s[0]} == {(38, 58, 12), (41, 58, 12), (76, 96, 12), (30, 50, 8), (33, 50, 8), (60, 80, 8)}
    assert {(o, a) for o, oc, a in fused._SUPPORTED if oc == o} == {(76, 12), (84, 12), (38, 12), (42, 12), (60, 8), (68, 8), (30, 8), (34, 8),
                                                                    (41, 12), (45, 12), (33, 8), (37, 8)}
    assert len(fused._SUPPORTED) == 18
    assert not fused.policy_kernels_supported(_policy())     # (parameters on the CPU: never)


def test_launcher_flag_and_example_file(tmp_path):
    import sys
    sys.path.insert(0, ROOT)
    import train_ppo
    path = os.path.join(ROOT, "configs", "critic_walk12.yaml")
    assert train_ppo.get_ppo_args([]).privileged_critic is None
    assert train_ppo.get_ppo_args(["--privileged-critic"]).privileged_critic is True
    assert train_ppo.get_ppo_args(["--privileged-critic", path]).privileged_critic == path
    cfg = os.path.join(ROOT, "configs", "basic12.yaml")
    from solorl_amd.config import load_yaml
    d = train_ppo.load_privileged_critic(path, load_yaml(cfg))
    assert d["command"] == [2.0, 2.0, 0.25]
    bad = tmp_path / "bad.yaml"
    bad.write_text("foot_farce: 1.0\n")
    with pytest.raises(SystemExit, match="foot_farce"):
        train_ppo.main(["--config-file", cfg, "--privileged-critic", str(bad)])
    with pytest.raises(SystemExit, match="--normalize-obs"):
        train_ppo.main(["--config-file", cfg, "--privileged-critic", "--normalize-obs"])
