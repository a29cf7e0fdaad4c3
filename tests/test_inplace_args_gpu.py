"""The in-place entry points of SoloVecEnv hand raw pointers to the C ABI, so every output tensor is checked on the host first: a wrong
dtype, a non-contiguous view, a missing row or a CPU tensor raises AssertionError naming the argument BEFORE anything is launched or
counted, and a correct call afterwards works with rewards (values, log-probs) in either shape [.., N] or [.., N, 1]."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, K = 5, 2


def _wrong(x, how):
    """`x` (a correct output tensor) made unacceptable in one way"""
    if how == "float64":
        return x.double()
    if how == "non_contiguous":
        return torch.zeros(x.shape[:-1] + (2 * x.shape[-1],), dtype=x.dtype, device=x.device)[..., ::2]
    if how == "row_short":
        return x[:-1]
    if how == "cpu":
        return x.cpu()
    raise KeyError(how)


HOW = ("float64", "non_contiguous", "row_short", "cpu")


@pytest.fixture(scope="module")
def stand8(gpu_device):
    from solorl_amd.config import default_config, ROBOT_SOLO8, TASK_STAND
    from solorl_amd.ppo import Policy
    from solorl_amd.ppo.fused import policy_params
    from solorl_amd.vec_env import Box, SoloVecEnv
    cfg = default_config(ROBOT_SOLO8, TASK_STAND)
    cfg.num_history_stack = 1
    env = SoloVecEnv(cfg, N, device=gpu_device, seed=4)
    env.reset()
    torch.manual_seed(2)
    pol = Policy((env.obs_dim,), Box(-np.ones(env.act_dim), np.ones(env.act_dim)), None, {"hidden_size": 64}).to(gpu_device)
    P = policy_params(pol)
    assert env.rollout_supported(P)
    yield env, P
    env.close()


def _entries(env, P, dev, tail):
    """name -> (call(**outputs), the correct output tensors by argument name, steps one call issues); `tail`: the trailing shape of the
    reward, value and log-prob rows, () or (1,)"""
    O, A = env.obs_dim, env.act_dim
    f32 = dict(dtype=torch.float32, device=dev)

    def rows(*lead):
        return dict(obs_out=torch.zeros(lead + (N, O), **f32), rew_out=torch.zeros(lead + (N,) + tail, **f32),
                    done_out=torch.zeros(lead + (N,), dtype=torch.uint8, device=dev))

    a1, aK, aK1 = torch.zeros(N, A, **f32), torch.zeros(K, N, A, **f32), torch.zeros(K + 1, N, A, **f32)
    out = {
        "step_inplace": (lambda **o: env.step_inplace(a1, **o), rows(), 1),
        "step_act_inplace": (lambda **o: env.step_act_inplace(a1, P, None, **o),
                             dict(rows(), value_out=torch.zeros((N,) + tail, **f32), action_out=torch.zeros(N, A, **f32),
                                  logp_out=torch.zeros((N,) + tail, **f32)), 1),
        "step_n_inplace": (lambda **o: env.step_n_inplace(aK, **o), rows(K), K),
        "rollout_inplace": (lambda **o: env.rollout_inplace(aK, P, None, **o),
                            dict(rows(K), value_out=torch.zeros((K, N) + tail, **f32), logp_out=torch.zeros((K, N) + tail, **f32)), K),
        "rollout_inplace_after_last": (lambda **o: env.rollout_inplace(aK1, P, None, policy_after_last=True, **o),
                                       dict(rows(K), value_out=torch.zeros((K + 1, N) + tail, **f32),
                                            logp_out=torch.zeros((K + 1, N) + tail, **f32)), K),
    }
    return out


@pytest.mark.parametrize("entry", ["step_inplace", "step_act_inplace", "step_n_inplace", "rollout_inplace", "rollout_inplace_after_last"])
def test_wrong_output_tensor_is_named_and_nothing_runs(stand8, gpu_device, entry):
    env, P = stand8
    call, good, steps = _entries(env, P, gpu_device, ())[entry]
    before, issued = env.get_states().bytes().clone(), env._steps_issued
    for name in good:
        for how in HOW:
            args = dict(good)
            args[name] = _wrong(good[name], how)
            with pytest.raises(AssertionError, match=name):
                call(**args)
    assert env._steps_issued == issued
    assert torch.equal(env.get_states().bytes(), before)     # bitwise: nothing was launched
    # a correct call afterwards works, with the rows in either accepted shape, and with the engine's own buffers
    for tail in ((), (1,)):
        call, good, steps = _entries(env, P, gpu_device, tail)[entry]
        o, r, d, info = call(**good)
        assert o is good["obs_out"] and r is good["rew_out"] and d is good["done_out"]
        issued += steps
        assert env._steps_issued == issued
        assert torch.isfinite(o).all() and bool((o != 0).any()) and torch.isfinite(r).all()
    o, r, d, info = call(**{k: v for k, v in good.items() if k not in ("obs_out", "rew_out", "done_out")})
    assert env._steps_issued == issued + steps
    assert o.shape == good["obs_out"].shape and d.dtype == torch.uint8 and torch.isfinite(o).all()
    assert not torch.equal(env.get_states().bytes(), before)
