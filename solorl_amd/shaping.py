"""Shaped reward terms of a whole batch: ``solorl_shape_reward`` (include/solorl.h, which holds the term table) from torch.

``shape_reward(cfg, params, states, actions, done, mem, reward)`` adds sixteen weighted terms -- base motion, torques, joint
acceleration, action rate, power, foot slip, clearance, contact force, air time, collisions, command tracking -- of the state rows
AFTER a step to that step's reward, in one kernel launch on the current stream, and keeps what the terms need of the previous step in
``mem``, a ``ShapeMem`` (one ``solorl_env_shape`` row per env).  ``SoloVecEnv.set_reward_shaping`` is the same call behind every step.
Every offset and shape is taken from the ctypes mirrors; none is written down here.
"""
import ctypes as C

import torch

from . import _native
from .rows import RowBatch, known_keys, mask_arg, members_of, state_rows, tensor_arg

TERMS = ("lin_vel_z", "ang_vel_xy", "orientation", "base_height", "torques", "joint_vel", "joint_acc", "action_rate", "power",
         "foot_slip", "foot_clearance", "foot_force", "feet_air_time", "collision", "tracking_lin_vel", "tracking_yaw_rate")
SHAPE_TERMS = len(TERMS)            # SOLORL_SHAPE_TERMS
EP_FIELDS = 1 + SHAPE_TERMS         # ep_out [17, N]: finished episodes, then each term's weighted sum over them
ENVS_PER_WORKGROUP = 64             # SHAPE_ENVS of csrc/solorl_shape.hip: rows one workgroup stages through LDS (a test shape, nothing else depends on it)


class ShapeParams(C.Structure):
    """ctypes mirror of ``solorl_shape_params``."""
    _fields_ = [("weight", C.c_double * SHAPE_TERMS), ("base_height_target", C.c_double), ("foot_clearance_target", C.c_double),
                ("foot_force_max", C.c_double), ("air_time_target", C.c_double), ("cmd_lin_vel", C.c_double * 2), ("cmd_yaw_rate", C.c_double),
                ("tracking_sigma", C.c_double)]


class EnvShape(C.Structure):
    """ctypes mirror of ``solorl_env_shape``."""
    _fields_ = [("prev_action", C.c_double * 12), ("prev_qd", C.c_double * 12), ("air_time", C.c_double * 4), ("ep_sum", C.c_double * SHAPE_TERMS),
                ("prev_contact", C.c_int32), ("valid", C.c_int32)]


ROW_BYTES = C.sizeof(EnvShape)
ROW_WORDS = ROW_BYTES // 8
assert ROW_BYTES == 360
MEMBERS = members_of(EnvShape, int32=True)

# parameters other than the weights, with the defaults of make_params (a Solo standing at rest: base 0.24 m up)
PARAM_DEFAULTS = {"base_height_target": 0.24, "foot_clearance_target": 0.06, "foot_force_max": 25.0, "air_time_target": 0.25,
                  "cmd_lin_vel": (0.5, 0.0), "cmd_yaw_rate": 0.0, "tracking_sigma": 0.25}


def make_params(weights, **params):
    """``weights``: dict term name -> weight (terms not named are off); ``params``: the members of solorl_shape_params other than the
    weights (PARAM_DEFAULTS).  Unknown names are refused by name."""
    known_keys("reward shaping term", weights, TERMS)
    known_keys("reward shaping parameter", params, PARAM_DEFAULTS)
    p = ShapeParams()
    for k, name in enumerate(TERMS):
        p.weight[k] = float(weights.get(name, 0.0))
    for name, default in PARAM_DEFAULTS.items():
        v = params.get(name, default)
        if name == "cmd_lin_vel":
            p.cmd_lin_vel[0], p.cmd_lin_vel[1] = float(v[0]), float(v[1])
        else:
            setattr(p, name, float(v))
    return p


def params_from_dict(d):
    """A reward-shaping file's dict (``weights:`` and the parameters as top-level keys, configs/shaping_walk12.yaml) -> ShapeParams"""
    d = dict(d)
    weights = d.pop("weights", None)
    if not isinstance(weights, dict):
        raise ValueError("a reward shaping file needs a `weights:` mapping of term name -> weight")
    return make_params(weights, **d)


class ShapeMem(RowBatch):
    """``data``: float64 ``[N, 45]`` (contiguous), one ``solorl_env_shape`` row per env.  Views: ``prev_action [N,12]``, ``prev_qd [N,12]``,
    ``air_time [N,4]``, ``ep_sum [N,16]`` (float64) and ``prev_contact [N]``, ``valid [N]`` (int32).  A zeroed row is an env at the start of
    an episode."""
    MIRROR = EnvShape


def shape_reward(cfg, params, states, actions, done, mem, reward, terms_out=None, ep_out=None, mask=None, commands=None):
    """``solorl_shape_reward`` on the rows of ``states`` (a StateBatch on a GPU: the state AFTER the step): ``actions`` float32 [N, A] (the
    step's raw actions), ``done`` uint8 [N] or None, ``mem`` a ShapeMem (read and rewritten), ``reward`` float32 [N] or [N, 1] (added to in
    place) or None, ``terms_out`` float64 [N, 16] or None (raw term values), ``ep_out`` float64 [17, N] or None (finished episodes'
    sums, accumulated), ``mask`` a [N] torch.bool / torch.uint8 tensor (rows whose byte is 0 are neither read nor written),
    ``commands`` a command.CommandMem of N rows or None: with rows the two tracking terms of env i compare it against its own command
    (``solorl_shape_reward_cmd``), without them against the one command of ``params``.  One launch on the current stream, no host
    synchronisation: capturable."""
    if not isinstance(params, ShapeParams) or not isinstance(mem, ShapeMem):
        raise AssertionError("params must be a ShapeParams and mem a ShapeMem")
    d, n, dev = state_rows("shape_reward", cfg, states)
    if not (mem.data.device == dev and mem.data.shape[0] == n):
        raise AssertionError("mem must hold %d rows on %s" % (n, dev))
    pa = tensor_arg("actions", actions, ((n, cfg.n_joints),), torch.float32, dev, optional=True)
    pd = tensor_arg("done", done, ((n,),), torch.uint8, dev, optional=True)
    pr = tensor_arg("reward", reward, ((n,), (n, 1)), torch.float32, dev, optional=True)
    pt = tensor_arg("terms_out", terms_out, ((n, SHAPE_TERMS),), torch.float64, dev, optional=True)
    pe = tensor_arg("ep_out", ep_out, ((EP_FIELDS, n),), torch.float64, dev, optional=True)
    m, pm = mask_arg(mask, n, dev)
    args = (C.byref(cfg), C.byref(params), C.c_void_p(d.data_ptr()), pm, n, pa, pd, C.c_void_p(mem.data.data_ptr()), pr, pt, pe)
    with torch.cuda.device(d.device):
        tail = (torch.cuda.current_device(), _native.stream(d.device))
        if commands is None:
            _native.check(_native.lib().solorl_shape_reward(*args, *tail))
        else:
            from .command import CommandMem
            if not (isinstance(commands, CommandMem) and commands.data.device == d.device and commands.data.shape[0] == n):
                raise AssertionError("commands must be a CommandMem of %d rows on %s" % (n, d.device))
            _native.check(_native.lib().solorl_shape_reward_cmd(*args, C.c_void_p(commands.data.data_ptr()), *tail))
    return reward
