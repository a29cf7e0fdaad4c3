"""The policy kernels (csrc/solorl_ppo.hip) at the observation widths of a commanded task without history: the engine's 38 / 42 (Solo12)
and 30 / 34 (Solo8) words plus the three command words of solorl_commands -- odd widths, which the kernels read word by word.
solorl_policy_act and the gradient stages against the PyTorch path at (45, 12) and (37, 8), with the bounds and the smallest batch sizes
tests/test_train_gpu.py uses for (42, 12); and policy_kernels_supported on a policy built from a commanded env."""
import numpy as np
import pytest
import torch

from tests.test_train_gpu import _check_minibatch_grad, _random_policy

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("O,A", [(45, 12), (37, 8), (41, 12), (33, 8)])
def test_policy_act_kernel_matches_torch_at_the_commanded_widths(gpu_device, O, A):
    """as tests/test_train_gpu.py test_policy_act_kernel_matches_torch: 1000 rows (a ragged last tile), with noise and deterministic"""
    from solorl_amd.ppo.fused import policy_act, policy_params, policy_kernels_supported
    dev = torch.device("cuda:0")
    pol = _random_policy(dev, O, A)
    assert policy_kernels_supported(pol)
    P = policy_params(pol)
    n = 1000
    obs = torch.randn(n, O, device=dev)
    for noise in (torch.randn(n, A, device=dev), None):
        v0, a0, l0 = torch.empty(n, 1, device=dev), torch.empty(n, A, device=dev), torch.empty(n, 1, device=dev)
        pol.act_into(obs, v0, a0, l0, noise=noise if noise is not None else torch.zeros(n, A, device=dev))
        v1, a1, l1 = torch.full((n, 1), 7.0, device=dev), torch.full((n, A), 7.0, device=dev), torch.full((n, 1), 7.0, device=dev)
        policy_act(P, obs, noise, v1, a1, l1)
        assert torch.allclose(v0, v1, rtol=1e-4, atol=1e-5), (v0 - v1).abs().max().item()
        assert torch.allclose(a0, a1, rtol=1e-4, atol=1e-5), (a0 - a1).abs().max().item()
        assert torch.allclose(l0, l1, rtol=1e-4, atol=1e-4), (l0 - l1).abs().max().item()


@pytest.mark.parametrize("O,A,clipped", [(45, 12, False), (37, 8, True)])
def test_minibatch_grad_kernel_matches_autograd_at_the_commanded_widths(gpu_device, O, A, clipped):
    """solorl_ppo_grad_stage1 / stage2 against loss.backward(): every parameter's gradient and the three loss values, at the shape
    tests/test_train_gpu.py checks (42, 12) at (16 x 128 rows, a mini-batch of 1024 at offset 512)"""
    _check_minibatch_grad(O, A, clipped, 16, 128, 1024, 512)


def test_a_policy_built_from_a_commanded_env_stays_on_the_kernels(gpu_device):
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    from solorl_amd.ppo import Policy
    from solorl_amd.ppo.fused import policy_kernels_supported
    from solorl_amd.vec_env import SoloVecEnv
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    cfg.num_history_stack = 0
    env = SoloVecEnv(cfg, 8, device="cuda:0", seed=1, commands=dict(lin_vel_x=(-0.5, 1.0), yaw_rate=(-1.0, 1.0), interval=(2, 5)))
    assert (env.engine_obs_dim, env.obs_dim) == (38, 41)
    pol = Policy(env.observation_space.shape, env.action_space, None, {"hidden_size": 64}).to("cuda:0")
    assert policy_kernels_supported(pol)
    env.close()
    cfg.num_history_stack = 1                               # one history level: 79 words, the PyTorch path
    env = SoloVecEnv(cfg, 8, device="cuda:0", seed=1, commands=dict(lin_vel_x=(-0.5, 1.0), interval=(2, 5)))
    pol = Policy(env.observation_space.shape, env.action_space, None, {"hidden_size": 64}).to("cuda:0")
    assert env.obs_dim == 79 and not policy_kernels_supported(pol)
    env.close()
