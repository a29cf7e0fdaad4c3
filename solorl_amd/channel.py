"""Observation noise and actuation of a whole batch: ``solorl_obs_noise`` and ``solorl_actuate`` (include/solorl.h, which holds both
draw tables) from torch.

``obs_noise(seed, env_id_offset, scale, count, obs)`` adds uniform noise of half-width ``scale[c]`` to component c of every observation
row; ``actuate(params, mem, actions)`` turns the policy's raw actions into what the motors receive -- delayed by a latency drawn per env
and episode, scaled by gains drawn per env, episode and joint -- with the per-env memory in ``mem``, an ``ActuatorMem`` (one
``solorl_env_actuator`` row per env).  Both are one kernel launch on the current stream, handle-free and keyed by seed and global env
id.  ``SoloVecEnv.set_obs_noise`` / ``set_actuation`` are the same calls around every step.  ``noise_scales`` builds the scale vector
from physical units per group of the observation.  Every offset is taken from the ctypes mirrors; none is written down here.
"""
import ctypes as C

import numpy as np
import torch

from . import _native
from ._native import Actuation, EnvActuator, DELAY_MAX
from .config import SoloConfig, TASK_POINTGOAL
from .rows import RowBatch, known_keys, mask_arg, tensor_arg

MAX_OBS = 210                       # 42 words x (1 + 4 history levels): the widest observation row
ROW_BYTES = C.sizeof(EnvActuator)
ROW_WORDS = ROW_BYTES // 4
assert ROW_BYTES == 256

# group of the observation -> what one unit of the observation is in the group's physical unit (oracle/solo_oracle.c current_state;
# `joint_pos` divides by the config's joint_limit)
GROUPS = ("height", "orientation", "lin_vel", "ang_vel", "joint_pos", "joint_vel", "position")


def group_layout(cfg):
    """[(group or None, first component, components, divisor)] of ONE level of the observation (``cfg.state_dim`` components): height,
    orientation (roll, pitch, yaw as (e mod 2) / 2), linear and angular velocity, joint positions / joint_limit, joint velocities / 100,
    the four feet flags and, for pointgoal, position xy / 2 and goal xy / 2.  None: a group that takes no noise (flags, goal)."""
    n = cfg.n_joints
    out = [("height", 0, 1, 1.0), ("orientation", 1, 3, 2.0), ("lin_vel", 4, 3, 1.0), ("ang_vel", 7, 3, 1.0),
           ("joint_pos", 10, n, float(cfg.joint_limit)), ("joint_vel", 10 + n, n, 100.0), (None, 10 + 2 * n, 4, 1.0)]
    if cfg.task == TASK_POINTGOAL:
        out += [("position", 14 + 2 * n, 2, 2.0), (None, 16 + 2 * n, 2, 2.0)]
    assert out[-1][1] + out[-1][2] == cfg.state_dim
    return out


def noise_scales(cfg, groups, history=1.0):
    """The ``[obs_dim]`` float32 scale vector (on the host) of ``solorl_obs_noise`` from half-widths in PHYSICAL units per group:
    ``groups`` maps height [m], orientation [rad], lin_vel [m/s], ang_vel [rad/s], joint_pos [rad], joint_vel [rad/s], position [m]
    (pointgoal xy) to a half-width; groups not named, the feet flags and the goal get 0.  Each is divided by the observation's own
    scaling: 1 for height and the velocities, 2 for orientation (the observation is (e mod 2) / 2, not e / 2 pi), joint_limit for joint
    positions, 100 for joint velocities, 2 for the position.  Each history difference block gets the level-0 scales times ``history``
    (every call draws every component anew: the noise of a difference block is not the difference of two levels' noise).
    The noise is additive and the wrapped orientation is NOT re-wrapped: a noisy angle component may leave [0, 1)."""
    if not isinstance(cfg, SoloConfig):
        raise AssertionError("cfg must be a SoloConfig")
    known_keys("observation noise group", groups, GROUPS)
    if "position" in groups and cfg.task != TASK_POINTGOAL:
        raise ValueError("observation noise group 'position' exists in the pointgoal observation only")
    level = np.zeros(cfg.state_dim, dtype=np.float64)
    for name, first, count, div in group_layout(cfg):
        if name is not None and name in groups:
            v = float(groups[name])
            if not (np.isfinite(v) and v >= 0.0):
                raise ValueError("observation noise of group %r must be finite and >= 0, got %r" % (name, groups[name]))
            level[first:first + count] = v / div
    out = np.concatenate([level] + [level * float(history)] * cfg.num_history_stack)
    return torch.from_numpy(out.astype(np.float32))


def scales_from_dict(cfg, d):
    """An observation-noise file's dict (``groups:`` and optionally ``history:``, configs/noise_solo.yaml) -> the scale vector"""
    d = dict(d)
    groups = d.pop("groups", None)
    if not isinstance(groups, dict):
        raise ValueError("an observation noise file needs a `groups:` mapping of group name -> half-width")
    history = d.pop("history", 1.0)
    known_keys("observation noise key", d, ("groups", "history"))
    return noise_scales(cfg, groups, history)


class ActuatorMem(RowBatch):
    """``data``: float32 ``[N, 64]`` (contiguous), one ``solorl_env_actuator`` row per env.  Views: ``buf [N,4,12]`` (level k = the raw
    action received k + 1 calls ago), ``gain [N,12]`` (float32) and ``latency [N]``, ``fill [N]``, ``episodes [N]`` (int32 views; episodes
    is the engine's uint32).  A zeroed row is an env that has drawn nothing yet: it draws at its first call."""
    MIRROR = EnvActuator
    WORD = torch.float32


def make_actuation(seed, env_id_offset, act_dim, delay=0, gain_range=0.0):
    """``solorl_actuation`` from ``delay`` (an int, or a (lo, hi) pair of control steps, 0 <= lo <= hi <= 4) and ``gain_range``"""
    lo, hi = (delay, delay) if np.isscalar(delay) else delay
    if int(lo) != lo or int(hi) != hi:
        raise AssertionError("delay must be an int or a pair of ints, got %r" % (delay,))
    return Actuation(int(seed) & (2 ** 64 - 1), int(env_id_offset), int(act_dim), int(lo), int(hi), 0, float(gain_range))


def obs_noise(seed, env_id_offset, scale, count, obs, out=None, mask=None):
    """``solorl_obs_noise``: ``obs`` float32 [n, D] on a GPU (dense rows; its first element need not be 16-byte aligned), ``scale`` float32
    [D], ``count`` int32 [n] (the engine's uint32 words: the noise calls each env has received, advanced by one for every live row),
    ``out`` = where the noisy rows go (default: in place), ``mask`` a [n] torch.bool / torch.uint8 tensor (rows whose byte is 0 are
    neither read nor written and their count stays).  One launch on the current stream, no host synchronisation: capturable."""
    if not (isinstance(obs, torch.Tensor) and obs.dim() == 2):
        raise AssertionError("obs must be a float32 [n, D] tensor, got %r" % (tuple(obs.shape) if isinstance(obs, torch.Tensor) else obs,))
    dev = obs.device if obs.is_cuda or not isinstance(count, torch.Tensor) else count.device     # (obs alone on the host is a bad argument)
    if dev.type != "cuda":
        raise _native.SoloRLError("obs_noise() needs observation rows [n, D] on a GPU (there is no CPU fallback)")
    n, D = obs.shape
    out = obs if out is None else out
    po, pq = tensor_arg("obs", obs, ((n, D),), torch.float32, dev), tensor_arg("out", out, ((n, D),), torch.float32, dev)
    ps = tensor_arg("scale", scale, ((D,),), torch.float32, dev)
    pc = tensor_arg("count", count, ((n,),), torch.int32, dev)
    m, pm = mask_arg(mask, n, dev)
    with torch.cuda.device(dev):
        _native.check(_native.lib().solorl_obs_noise(int(seed) & (2 ** 64 - 1), int(env_id_offset), ps, pm, n, D, pc,
                                                     po, pq, torch.cuda.current_device(), _native.stream(dev)))
    return out


def actuate(params, mem, actions, out=None, restart=None):
    """``solorl_actuate``: ``params`` an Actuation (make_actuation), ``mem`` an ActuatorMem of n rows (read and rewritten), ``actions``
    float32 [n, A] (the raw actions), ``out`` = where the applied actions go (default: a new tensor; may be ``actions``), ``restart`` a [n]
    torch.bool / torch.uint8 tensor (envs that start an episode with this action) or None.  One launch on the current stream, no host
    synchronisation: capturable."""
    if not isinstance(params, Actuation) or not isinstance(mem, ActuatorMem):
        raise AssertionError("params must be an Actuation and mem an ActuatorMem")
    d = mem.data
    n = d.shape[0]
    if not d.is_cuda:
        raise _native.SoloRLError("actuate() needs its memory rows on a GPU (there is no CPU fallback)")
    pa = tensor_arg("actions", actions, ((n, params.act_dim),), torch.float32, d.device)
    if out is None:
        out = torch.empty_like(actions)
    po = tensor_arg("out", out, ((n, params.act_dim),), torch.float32, d.device)
    r, pr = mask_arg(restart, n, d.device, "restart")
    with torch.cuda.device(d.device):
        _native.check(_native.lib().solorl_actuate(C.byref(params), n, pr, C.c_void_p(d.data_ptr()), pa, po, torch.cuda.current_device(),
                                                   _native.stream(d.device)))
    return out
