"""Privileged critic rows of a whole batch: ``solorl_critic_obs`` (include/solorl.h, which holds the word table) from torch.

``critic_obs(cfg, params, states, obs)`` returns, for every env, the clean observation row followed by twenty words of the simulator's
truth -- the four feet's contact forces, heights and horizontal speeds, the env's velocity command, the episode's progress, the number
of colliding primitives, the actuation latency and mean gain error that were drawn, and the size of the last kick -- each scaled by
``params.scale``.  One kernel launch on the current stream, handle-free.  ``SoloVecEnv(..., critic_obs=True)`` is the same call behind
every step and reset.  ``scales_from_dict`` reads a scale file's dict (configs/critic_walk12.yaml).
"""
import ctypes as C

import numpy as np
import torch

from . import _native
from ._native import CRITIC_PRIV, CriticParams
from .rows import known_keys, mask_arg, state_rows, tensor_arg

MAX_OBS = 210                       # the widest observation row the call takes
ENVS_PER_WORKGROUP = 64             # CRITIC_ENVS of csrc/solorl_critic.hip: rows one workgroup stages through LDS (a test shape, nothing else depends on it)

# group of privileged words -> (first word, words), in the order of the table of include/solorl.h
GROUPS = {"foot_force": (0, 4), "foot_height": (4, 4), "foot_speed": (8, 4), "command": (12, 3), "time": (15, 1), "collisions": (16, 1),
          "latency": (17, 1), "gain": (18, 1), "kick": (19, 1)}
assert sum(k for _, k in GROUPS.values()) == CRITIC_PRIV


def default_scales(cfg):
    """Untuned factors that bring every word to the order of 1: forces / 20 N, heights x 10 (feet swing a few cm), speeds and commands
    as they are (m/s, rad/s), the time step / episode_length, collisions / 4, the latency / SOLORL_DELAY_MAX, the mean gain error x 5,
    the kick as it is (m/s)."""
    return {"foot_force": 0.05, "foot_height": 10.0, "foot_speed": 1.0, "command": 1.0, "time": 1.0 / max(1, int(cfg.episode_length)),
            "collisions": 0.25, "latency": 1.0 / _native.DELAY_MAX, "gain": 5.0, "kick": 1.0}


def make_params(cfg, obs_dim, **scales):
    """``solorl_critic_params`` for observation rows of ``obs_dim`` words: ``scales`` maps a group of GROUPS to one factor for all of its
    words or to one factor per word; groups not named take ``default_scales(cfg)``.  Unknown names are refused by name."""
    known_keys("critic scale", scales, GROUPS)
    p = CriticParams()
    p.obs_dim = int(obs_dim)
    if not 1 <= p.obs_dim <= MAX_OBS:
        raise ValueError("critic rows take observation rows of 1..%d words, got %r" % (MAX_OBS, obs_dim))
    for name, v in dict(default_scales(cfg), **scales).items():
        first, count = GROUPS[name]
        v = np.broadcast_to(np.asarray(v, dtype=np.float64), (count,)) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)
        if v.shape != (count,) or not np.isfinite(v).all():
            raise ValueError("critic scale %r must be one finite factor or %d of them, got %r" % (name, count, scales.get(name)))
        for k in range(count):
            p.scale[first + k] = float(v[k])
    return p


def scales_from_dict(d):
    """A scale file's dict (configs/critic_walk12.yaml: group name -> factor or list of factors) -> the keyword arguments of make_params,
    unknown keys refused by name"""
    if not isinstance(d, dict):
        raise ValueError("a critic scale file holds a mapping with the keys %s" % ", ".join(GROUPS))
    known_keys("critic scale", d, GROUPS)
    return dict(d)


def critic_obs(cfg, params, states, obs, out=None, commands=None, actuators=None, kick=None, mask=None):
    """``solorl_critic_obs`` on the rows of ``states`` (a StateBatch on a GPU: the state the observation describes): ``params`` a
    CriticParams (make_params), ``obs`` float32 [n, E] (E = params.obs_dim: the engine's clean rows), ``out`` float32 [n, E + 20]
    (default: a new tensor; it must not overlap ``obs``), ``commands`` a command.CommandMem of n rows or None, ``actuators`` a
    channel.ActuatorMem of n rows or None, ``kick`` float64 [n, 6] (SoloVecEnv.last_kick) or None, ``mask`` a [n] torch.bool / torch.uint8
    tensor (rows whose byte is 0 are neither read nor written).  -> ``out``.  One launch on the current stream, no host
    synchronisation: capturable."""
    if not isinstance(params, CriticParams):
        raise AssertionError("params must be a CriticParams")
    d, n, dev = state_rows("critic_obs", cfg, states)
    E = params.obs_dim
    po = tensor_arg("obs", obs, ((n, E),), torch.float32, dev)
    if out is None:
        out = torch.empty((n, E + CRITIC_PRIV), dtype=torch.float32, device=dev)
    pq = tensor_arg("out", out, ((n, E + CRITIC_PRIV),), torch.float32, dev)
    pc, pa = C.c_void_p(0), C.c_void_p(0)
    if commands is not None:
        from .command import CommandMem
        if not (isinstance(commands, CommandMem) and commands.data.device == dev and commands.data.shape[0] == n):
            raise AssertionError("commands must be a CommandMem of %d rows on %s" % (n, dev))
        pc = C.c_void_p(commands.data.data_ptr())
    if actuators is not None:
        from .channel import ActuatorMem
        if not (isinstance(actuators, ActuatorMem) and actuators.data.device == dev and actuators.data.shape[0] == n):
            raise AssertionError("actuators must be an ActuatorMem of %d rows on %s" % (n, dev))
        pa = C.c_void_p(actuators.data.data_ptr())
    pk = tensor_arg("kick", kick, ((n, 6),), torch.float64, dev, optional=True)
    m, pm = mask_arg(mask, n, dev)
    with torch.cuda.device(dev):
        _native.check(_native.lib().solorl_critic_obs(C.byref(cfg), C.byref(params), C.c_void_p(d.data_ptr()), pm, n, po, pc, pa, pk, pq,
                                                      torch.cuda.current_device(), _native.stream(dev)))
    return out
