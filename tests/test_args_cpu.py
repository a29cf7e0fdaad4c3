"""The shared pieces of the Python layer without a GPU (solorl_amd/rows.py, the stage table of solorl_amd/vec_env.py): the one check of a
raw-pointer argument, the one unknown-key refusal with the message text each of its sites has always had, the per-env memory classes
laid over the ctypes mirrors, and which stages bar which launches."""
import ctypes as C
import struct
import types

import pytest
import torch

from solorl_amd import _native, channel, command, reset_random, shaping, termination
from solorl_amd.config import ROBOT_SOLO12, TASK_WALK, default_config
from solorl_amd.rows import known_keys, tensor_arg
from solorl_amd.vec_env import SoloVecEnv

DEV = torch.device("cuda", 0)       # (never touched: every check below ends before a device is asked for)


# ---------------------------------------------------------------- tensor_arg
def _strided():
    return torch.zeros(4, 6)[:, ::2]


@pytest.mark.parametrize("x, device, what", [
    (torch.zeros(4, 3), DEV, "on cpu"),                                 # on another device
    (torch.zeros(4, 3, dtype=torch.float64), "cpu", "torch.float64"),   # wrong dtype
    (torch.zeros(4, 2), "cpu", "(4, 2)"),                               # wrong shape
    (_strided(), "cpu", "not contiguous"),                              # right shape, not contiguous
    ([[0.0] * 3] * 4, "cpu", "a list"),                                 # no tensor
    (None, "cpu", "None"),                                              # None without optional
])
def test_tensor_arg_refuses_by_name_and_says_what_it_got(x, device, what):
    with pytest.raises(AssertionError) as e:
        tensor_arg("reward_out", x, ((4, 3), (4, 3, 1)), torch.float32, torch.device(device))
    msg = str(e.value)
    assert msg.startswith("reward_out must be a contiguous float32 [4, 3] or [4, 3, 1] tensor on %s, got " % torch.device(device)), msg
    assert what in msg.split(", got ")[1], msg


def test_tensor_arg_accepts_and_gives_the_pointer():
    x = torch.zeros(4, 3, 1)
    p = tensor_arg("x", x, ((4, 3), (4, 3, 1)), torch.float32, torch.device("cpu"))
    assert isinstance(p, C.c_void_p) and p.value == x.data_ptr()
    p = tensor_arg("x", None, ((4, 3),), torch.float32, DEV, optional=True)
    assert isinstance(p, C.c_void_p) and not p.value                    # a null pointer
    with pytest.raises(AssertionError, match="x must be"):              # optional lets None through and nothing else
        tensor_arg("x", torch.zeros(4, 2), ((4, 3),), torch.float32, torch.device("cpu"), optional=True)


# ---------------------------------------------------------------- known_keys
_CMD = "lin_vel_x, lin_vel_y, yaw_rate, interval, zero_prob, min_lin_norm, obs_scale"
_TERM = "base_height, max_tilt_deg, contacts, contact_force_min, joint_limits, min_steps, terminal_reward"
_RESET = "joint_pos, joint_vel, lin_vel, ang_vel, yaw, roll, pitch, clearance, place_on_ground"
_TERMS = ("lin_vel_z, ang_vel_xy, orientation, base_height, torques, joint_vel, joint_acc, action_rate, power, foot_slip, foot_clearance, "
          "foot_force, feet_air_time, collision, tracking_lin_vel, tracking_yaw_rate")
_PARAMS = "base_height_target, foot_clearance_target, foot_force_max, air_time_target, cmd_lin_vel, cmd_yaw_rate, tracking_sigma"
_CFG = default_config(ROBOT_SOLO12, TASK_WALK)

# the nine sites (and the observation noise groups), each with the text it raised before there was one known_keys
SITES = [
    (lambda: command.make_params(0, 0, 1, lin_vel_z=1.0), "unknown command key(s) 'lin_vel_z' (known: %s)" % _CMD),
    (lambda: command.ranges_from_dict({"yaw_rat": [0, 1]}), "unknown command key(s) 'yaw_rat' (known: %s)" % _CMD),
    (lambda: termination.make_termination(ROBOT_SOLO12, base_hight=0.1), "unknown termination key(s) 'base_hight' (known: %s)" % _TERM),
    (lambda: termination.rules_from_dict({"max_tilt": 60}), "unknown termination key(s) 'max_tilt' (known: %s)" % _TERM),
    (lambda: reset_random.make_reset_randomization(_CFG, 0, 0, jointpos=0.1), "unknown reset randomization key(s) 'jointpos' (known: %s)" % _RESET),
    (lambda: reset_random.ranges_from_dict({"heading": 3.0}), "unknown reset randomization key(s) 'heading' (known: %s)" % _RESET),
    (lambda: shaping.make_params({"foot_slop": 1.0}), "unknown reward shaping term(s) 'foot_slop' (known: %s)" % _TERMS),
    (lambda: shaping.make_params({"foot_slip": 1.0}, sigma=0.5), "unknown reward shaping parameter(s) 'sigma' (known: %s)" % _PARAMS),
    (lambda: channel.scales_from_dict(_CFG, {"groups": {}, "histroy": 2.0}), "unknown observation noise key(s) 'histroy' (known: groups, history)"),
    (lambda: channel.noise_scales(_CFG, {"hieght": 0.01}),
     "unknown observation noise group(s) 'hieght' (known: height, orientation, lin_vel, ang_vel, joint_pos, joint_vel, position)"),
]


@pytest.mark.parametrize("k", range(len(SITES)))
def test_unknown_keys_are_refused_with_the_text_each_site_has_always_had(k):
    call, text = SITES[k]
    with pytest.raises(ValueError) as e:
        call()
    assert str(e.value) == text


def test_known_keys_sorts_and_quotes_and_passes_what_is_known():
    known_keys("thing", {"a": 1}, ("a", "b"))
    known_keys("thing", (), ("a", "b"))
    with pytest.raises(ValueError) as e:
        known_keys("thing", {"z": 1, "a": 2, "c": 3}, ("a", "b"))
    assert str(e.value) == "unknown thing(s) 'c', 'z' (known: a, b)"


# ---------------------------------------------------------------- CommandMem, ActuatorMem
def _word(mem, row, offset, fmt):
    size = struct.calcsize(fmt)
    return struct.unpack(fmt, bytes(mem.bytes()[row, offset:offset + size].tolist()))[0]


def test_command_mem_views_lie_where_ctypes_says():
    E = _native.EnvCommand
    mem = command.CommandMem(4, "cpu")
    assert mem.num_envs == 4 and mem.data.dtype == torch.float64 and tuple(mem.data.shape) == (4, C.sizeof(E) // 8) == (4, 4)
    assert tuple(mem.cmd.shape) == (4, 3) and mem.cmd.dtype == torch.float64
    assert tuple(mem.countdown.shape) == tuple(mem.draws.shape) == (4,) and mem.countdown.dtype == mem.draws.dtype == torch.int32
    mem.cmd[1, 2] = 3.5
    mem.countdown[2] = 0x01020304
    mem.draws[3] = 0x0A0B0C0D
    assert _word(mem, 1, E.cmd.offset + 2 * 8, "<d") == 3.5
    assert _word(mem, 2, E.countdown.offset, "<i") == 0x01020304
    assert _word(mem, 3, E.draws.offset, "<i") == 0x0A0B0C0D
    assert int(mem.bytes().ne(0).sum()) == 2 + 4 + 4                    # (3.5 has two non-zero bytes) nothing else was written
    twin = mem.clone()
    assert type(twin) is command.CommandMem and torch.equal(twin.bytes(), mem.bytes()) and twin.data.data_ptr() != mem.data.data_ptr()
    assert tuple(mem.bytes().shape) == (4, 32) and mem.bytes().dtype == torch.uint8
    with pytest.raises(AssertionError, match="CommandMem data must be a contiguous float64"):
        command.CommandMem(data=torch.zeros(4, 4, dtype=torch.float32))


def test_actuator_mem_views_lie_where_ctypes_says():
    E = _native.EnvActuator
    mem = channel.ActuatorMem(4, "cpu")
    assert mem.num_envs == 4 and mem.data.dtype == torch.float32 and tuple(mem.data.shape) == (4, C.sizeof(E) // 4) == (4, 64)
    assert tuple(mem.buf.shape) == (4, _native.DELAY_MAX, 12) and tuple(mem.gain.shape) == (4, 12) and mem.buf.dtype == mem.gain.dtype == torch.float32
    for v in (mem.latency, mem.fill, mem.episodes):
        assert tuple(v.shape) == (4,) and v.dtype == torch.int32
    mem.buf[1, 2, 5] = 7.25
    mem.gain[2, 11] = -0.5
    mem.latency[0] = 0x01020304
    mem.fill[1] = 0x05060708
    mem.episodes[3] = 0x0A0B0C0D
    assert _word(mem, 1, E.buf.offset + (2 * 12 + 5) * 4, "<f") == 7.25
    assert _word(mem, 2, E.gain.offset + 11 * 4, "<f") == -0.5
    assert _word(mem, 0, E.latency.offset, "<i") == 0x01020304
    assert _word(mem, 1, E.fill.offset, "<i") == 0x05060708
    assert _word(mem, 3, E.episodes.offset, "<i") == 0x0A0B0C0D
    assert int(mem.bytes().ne(0).sum()) == 2 + 1 + 4 + 4 + 4            # (7.25: two non-zero bytes, -0.5: one) nothing else was written
    twin = mem.clone()
    assert type(twin) is channel.ActuatorMem and torch.equal(twin.bytes(), mem.bytes()) and twin.data.data_ptr() != mem.data.data_ptr()
    assert tuple(mem.bytes().shape) == (4, 256) and mem.bytes().dtype == torch.uint8
    with pytest.raises(AssertionError, match="ActuatorMem data must be a contiguous float32"):
        channel.ActuatorMem(data=torch.zeros(4, 64, dtype=torch.float64))


# ---------------------------------------------------------------- the stage table
# stage -> (the attribute that sets it, a value that does, does it bar K steps in one launch, does it bar the policy tail, a word of the
# message): what the guards did when each was written out by hand
STAGES = {
    "commands": ("_cmd", object(), True, True, "velocity commands"),
    "perturbation": ("last_kick", object(), True, False, "perturbation"),
    "actuation": ("_act", object(), True, False, "actuation"),
    "termination": ("_term", object(), True, True, "termination"),
    "shaping": ("_shape_params", object(), True, False, "reward shaping"),
    "reset randomization": ("_rr", object(), True, True, "reset randomization"),
    "noise": ("_noise_scale", object(), True, True, "observation noise"),
    "norm_obs": ("_norm_obs", True, False, True, "norm_obs"),
}
GUARDS = {"commands": "_no_commands", "perturbation": "_no_kicks", "actuation": "_no_channel", "termination": "_no_termination",
          "shaping": "_no_shaping", "reset randomization": "_no_reset_randomization", "noise": "_no_channel"}


def _fake(**on):
    """what the guards read of an env, everything off but ``on``; the handle says the policy tail is possible"""
    e = types.SimpleNamespace(_norm_obs=False, last_kick=None, _shape_params=None, _noise_scale=None, _act=None, _cmd=None, _term=None, _rr=None,
                              obs_dim=76, act_dim=12, get_property=lambda name: 1.0 if name == "step_n_one_launch" else 0.0)
    e.step_act_supported = lambda params: SoloVecEnv.step_act_supported(e, params)
    e._refuse = lambda *a, **kw: SoloVecEnv._refuse(e, *a, **kw)
    for k, v in on.items():
        setattr(e, k, v)
    return e


P = types.SimpleNamespace(obs_dim=76, act_dim=12, hidden=64)


def test_with_no_stage_set_nothing_is_refused():
    e = _fake()
    SoloVecEnv._refuse(e, "step_n", k_step=True)
    SoloVecEnv._refuse(e, "rollout_inplace", tail=True)
    SoloVecEnv._no_policy_tail(e, "step_act_inplace")
    for g in set(GUARDS.values()):
        getattr(SoloVecEnv, g)(e, "step_n")
    assert SoloVecEnv.step_act_supported(e, P) and SoloVecEnv.rollout_supported(e, P)


@pytest.mark.parametrize("stage", sorted(STAGES))
def test_each_stage_bars_what_it_always_barred(stage):
    attr, value, bars_k, bars_tail, word = STAGES[stage]
    e = _fake(**{attr: value})
    # K steps in one launch
    if bars_k:
        for name in ("step_n", "rollout_inplace"):
            with pytest.raises(_native.SoloRLError, match=r"%s.*%s(.|\n)*rollout_supported\(\) is False" % (name, word)):
                SoloVecEnv._refuse(e, name, k_step=True)
        with pytest.raises(_native.SoloRLError, match="step_n.*" + word):
            getattr(SoloVecEnv, GUARDS[stage])(e, "step_n")
    else:
        SoloVecEnv._refuse(e, "step_n", k_step=True)
    for other in set(GUARDS.values()) - {GUARDS.get(stage)}:           # no other stage's guard fires
        getattr(SoloVecEnv, other)(e, "step_n")
    # the policy inside the step kernel
    if bars_tail:
        for name in ("step_act_inplace", "rollout_inplace"):
            with pytest.raises(_native.SoloRLError, match=r"%s.*%s(.|\n)*step_act_supported\(\) / rollout_supported\(\) are False" % (name, word)):
                SoloVecEnv._no_policy_tail(e, name)
    else:
        SoloVecEnv._no_policy_tail(e, "step_act_inplace")
    assert SoloVecEnv.step_act_supported(e, P) == (not bars_tail)
    assert SoloVecEnv.rollout_supported(e, P) == (not bars_k and not bars_tail)
