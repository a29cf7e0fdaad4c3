"""Which native calls SoloVecEnv issues, and in which order, with every optional stage set -- the step chain is written once
(_before_step / _after_step), and these lists are what it has to come to: they were recorded with the same recorder on the code that
still wrote the chain out per entry point.  Then the wrappers' refusals: a bad tensor argument raises AssertionError naming it before
anything is launched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 8

RESET = ["solorl_reset", "solorl_get_states", "solorl_randomize_reset", "solorl_set_states", "solorl_restart_history", "solorl_obs_noise",
         "solorl_commands", "solorl_normalize_obs"]
STEP = ["solorl_actuate", "solorl_perturb", "solorl_step", "solorl_get_states", "solorl_terminate", "solorl_reset_masked",
        "solorl_shape_reward_cmd", "solorl_get_states", "solorl_randomize_reset", "solorl_set_states", "solorl_restart_history",
        "solorl_obs_noise", "solorl_commands", "solorl_normalize_obs", "solorl_normalize_rewards"]
RESET_MASKED = ["solorl_get_observation", "solorl_reset_masked", "solorl_get_states", "solorl_randomize_reset", "solorl_set_states",
                "solorl_restart_history", "solorl_obs_noise", "solorl_commands", "solorl_normalize_obs"]
STEP_ACT = ["solorl_actuate", "solorl_perturb", "solorl_step_act", "solorl_get_states", "solorl_shape_reward", "solorl_normalize_rewards"]


class Recorder:
    """Forwards to the loaded library and logs the name of every entry point called"""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if not name.startswith("solorl_"):
            return f

        def call(*args):
            self.calls.append(name)
            return f(*args)
        return call

    def during(self, fn):
        self.calls = []
        fn()
        return self.calls


@pytest.fixture
def recorder(monkeypatch):
    from solorl_amd import _native
    rec = Recorder(_native.lib())
    monkeypatch.setattr(_native, "_LIB", rec)      # before the env is built: env.L and the wrapper modules share it
    return rec


def _cfg():
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    cfg.num_history_stack = 1
    return cfg


def test_every_stage_set_the_calls_and_their_order(gpu_device, recorder):
    from solorl_amd.vec_env import SoloVecEnv
    env = SoloVecEnv(_cfg(), N, device=gpu_device, seed=3, norm_obs=True, norm_ret=True, commands={"lin_vel_x": [0.0, 1.0], "interval": [2, 5]})
    assert env.L is recorder
    env.set_perturbation((2, 4), 0.3, 0.3)
    env.set_actuation((0, 2), 0.1)
    env.set_termination(base_height=0.12, max_tilt_deg=60.0)
    env.set_reward_shaping({"foot_slip": -0.1, "tracking_lin_vel": 1.0})
    env.set_reset_randomization(joint_pos=0.1, yaw=1.0)
    env.set_obs_noise({"height": 0.01, "joint_pos": 0.01})
    a = torch.zeros(N, env.act_dim, device=gpu_device)
    mask = torch.zeros(N, dtype=torch.bool, device=gpu_device)
    mask[::3] = True
    assert recorder.during(env.reset) == RESET
    assert recorder.during(lambda: env.step(a)) == STEP
    assert recorder.during(lambda: env.step_inplace(a)) == STEP
    assert recorder.during(lambda: env.reset_masked(mask)) == RESET_MASKED
    assert env._steps_issued == 2
    torch.cuda.synchronize()
    env.close()


def test_the_policy_tail_with_the_stages_it_allows(gpu_device, recorder):
    import numpy as np
    from solorl_amd.ppo import Policy
    from solorl_amd.ppo.fused import policy_params
    from solorl_amd.vec_env import Box, SoloVecEnv
    env = SoloVecEnv(_cfg(), N, device=gpu_device, seed=3, norm_ret=True)
    env.set_perturbation((2, 4), 0.3, 0.3)
    env.set_actuation((0, 2), 0.1)
    env.set_reward_shaping({"foot_slip": -0.1, "action_rate": -0.01})
    torch.manual_seed(2)
    pol = Policy((env.obs_dim,), Box(-np.ones(env.act_dim), np.ones(env.act_dim)), None, {"hidden_size": 64}).to(gpu_device)
    P = policy_params(pol)
    assert env.step_act_supported(P) and not env.rollout_supported(P)
    env.reset()
    f32 = dict(dtype=torch.float32, device=gpu_device)
    a, v, act, lp = torch.zeros(N, env.act_dim, **f32), torch.zeros(N, **f32), torch.zeros(N, env.act_dim, **f32), torch.zeros(N, **f32)
    assert recorder.during(lambda: env.step_act_inplace(a, P, None, v, act, lp)) == STEP_ACT
    torch.cuda.synchronize()
    env.close()


# ---------------------------------------------------------------- refusals of the wrappers
n = 4


def _wrong(x, how):
    """`x` (a correct tensor argument) made unacceptable in one way"""
    if how == "dtype":
        return x.to(torch.float32 if x.dtype == torch.float64 else torch.float64)
    if how == "shape":                              # one row more
        return x.new_zeros((x.shape[0] + 1,) + tuple(x.shape[1:]))
    if how == "extra_dim":
        return x.unsqueeze(0).contiguous()
    if how == "non_contiguous":
        return x.new_zeros(tuple(x.shape[:-1]) + (2 * x.shape[-1],))[..., ::2]
    if how == "cpu":
        return x.cpu()
    raise KeyError(how)


def _calls(dev):
    """entry -> (call(**tensors), the correct tensor arguments by name, the other in/out tensors of the call)"""
    from solorl_amd import channel, command, reset_random, shaping, termination
    from solorl_amd.state import StateBatch
    from solorl_amd.vec_env import SoloVecEnv
    cfg = _cfg()
    env = SoloVecEnv(cfg, n, device=dev, seed=5)
    env.reset()
    states = env.get_states()
    env.close()
    assert isinstance(states, StateBatch)
    f32, f64, u8 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev), dict(dtype=torch.uint8, device=dev)
    A, D = cfg.n_joints, 76
    term = termination.make_termination(cfg, base_height=0.1)
    sp = shaping.make_params({"foot_slip": -0.1})
    smem = shaping.ShapeMem(n, dev)
    rr = reset_random.make_reset_randomization(cfg, 1, 0, joint_pos=0.1)
    cp = command.make_params(1, 0, D, lin_vel_x=[0.0, 1.0])
    cmem = command.CommandMem(n, dev)
    ap = channel.make_actuation(1, 0, A, (0, 2), 0.1)
    amem = channel.ActuatorMem(n, dev)
    ones = lambda: torch.ones(n, **u8)
    return {
        "terminate": (lambda **t: termination.terminate(cfg, term, states, t["done"], t["reward"], t["fired_out"], term_stats=t["term_stats"], mask=t["mask"]),
                      dict(done=torch.zeros(n, **u8), reward=torch.zeros(n, **f32), fired_out=torch.zeros(n, **u8),
                           term_stats=torch.zeros(termination.STAT_FIELDS, n, **f32), mask=ones()), [states.data]),
        "shape_reward": (lambda **t: shaping.shape_reward(cfg, sp, states, t["actions"], t["done"], smem, t["reward"], terms_out=t["terms_out"],
                                                          ep_out=t["ep_out"], mask=t["mask"]),
                         dict(actions=torch.zeros(n, A, **f32), done=torch.zeros(n, **u8), reward=torch.zeros(n, **f32),
                              terms_out=torch.zeros(n, shaping.SHAPE_TERMS, **f64), ep_out=torch.zeros(shaping.EP_FIELDS, n, **f64), mask=ones()),
                         [states.data, smem.data]),
        "randomize_reset": (lambda **t: reset_random.randomize_reset(cfg, rr, states, t["count"], mask=t["mask"]),
                            dict(count=torch.zeros(n, dtype=torch.int32, device=dev), mask=ones()), [states.data]),
        "commands": (lambda **t: command.commands(cp, cmem, t["obs"], out=t["out"], cmd_out=t["cmd_out"], restart=t["restart"], mask=t["mask"]),
                     dict(obs=torch.zeros(n, D, **f32), out=torch.zeros(n, D + 3, **f32), cmd_out=torch.zeros(n, 3, **f64), restart=ones(), mask=ones()),
                     [cmem.data]),
        "actuate": (lambda **t: channel.actuate(ap, amem, t["actions"], out=t["out"], restart=t["restart"]),
                    dict(actions=torch.ones(n, A, **f32), out=torch.zeros(n, A, **f32), restart=ones()), [amem.data]),
        "obs_noise": (lambda **t: channel.obs_noise(1, 0, t["scale"], t["count"], t["obs"], out=t["out"], mask=t["mask"]),
                      dict(scale=torch.full((D,), 0.01, **f32), count=torch.zeros(n, dtype=torch.int32, device=dev), obs=torch.zeros(n, D, **f32),
                           out=torch.zeros(n, D, **f32), mask=ones()), []),
    }


# obs_noise takes n and D from `obs` itself: a row more there makes `out` the argument that does not fit, so its wrong shape is a third dimension
HOW = {("obs_noise", "obs"): ("dtype", "extra_dim", "non_contiguous", "cpu")}


@pytest.mark.parametrize("entry", ["terminate", "shape_reward", "randomize_reset", "commands", "actuate", "obs_noise"])
def test_a_bad_tensor_argument_is_named_and_nothing_is_launched(gpu_device, entry):
    call, good, others = _calls(gpu_device)[entry]
    before = [t.clone() for t in list(good.values()) + others]
    for name in good:
        for how in HOW.get((entry, name), ("dtype", "shape", "non_contiguous", "cpu")):
            args = dict(good)
            args[name] = _wrong(good[name], how)
            with pytest.raises(AssertionError, match=r"^%s must be " % name):
                call(**args)
    torch.cuda.synchronize()
    for t, was in zip(list(good.values()) + others, before):
        assert torch.equal(t.view(torch.uint8), was.view(torch.uint8))          # bitwise: nothing was launched
    call(**good)                                                                # (the arguments the bad ones were made from are good)
    torch.cuda.synchronize()
