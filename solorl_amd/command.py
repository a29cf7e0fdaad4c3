"""Per-env velocity commands of a whole batch: ``solorl_commands`` (include/solorl.h, which holds the draw table) from torch.

``commands(params, mem, obs)`` lets every env whose countdown runs out draw a new command (vx, vy in m/s, a yaw rate in rad/s, base frame)
from the ranges in ``params`` and returns the observation rows widened by the three command words the policy is to see; the per-env
memory is ``mem``, a ``CommandMem`` (one ``solorl_env_command`` row per env).  One kernel launch on the current stream, handle-free and
keyed by seed and global env id.  ``SoloVecEnv(..., commands=)`` is the same call behind every step.  ``ranges_from_dict`` reads a
command file's dict (configs/commands_walk12.yaml).  Every offset is taken from the ctypes mirrors; none is written down here.
"""
import ctypes as C

import numpy as np
import torch

from . import _native
from ._native import CommandParams, EnvCommand
from .rows import RowBatch, known_keys, mask_arg, tensor_arg

MAX_OBS = 210                       # the widest observation row the call widens
INTERVAL_MAX = 1 << 20
ROW_BYTES = C.sizeof(EnvCommand)
ROW_WORDS = ROW_BYTES // 8
assert ROW_BYTES == 32

RANGE_KEYS = ("lin_vel_x", "lin_vel_y", "yaw_rate")
KEYS = RANGE_KEYS + ("interval", "zero_prob", "min_lin_norm", "obs_scale")
DEFAULTS = {"lin_vel_x": (0.0, 0.0), "lin_vel_y": (0.0, 0.0), "yaw_rate": (0.0, 0.0), "interval": 1, "zero_prob": 0.0, "min_lin_norm": 0.0,
            "obs_scale": (1.0, 1.0, 1.0)}


class CommandMem(RowBatch):
    """``data``: float64 ``[N, 4]`` (contiguous), one ``solorl_env_command`` row per env.  Views: ``cmd [N, 3]`` (float64) and
    ``countdown [N]``, ``draws [N]`` (int32 views; draws is the engine's uint32).  A zeroed row is an env that has drawn nothing yet: it
    draws at its first call."""
    MIRROR = EnvCommand


def _pair(name, v):
    lo, hi = (v, v) if np.isscalar(v) else v
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise ValueError("command range %r must be a finite [lo, hi] pair with lo <= hi, got %r" % (name, v))
    return lo, hi


def make_params(seed, env_id_offset, obs_dim, **ranges):
    """``solorl_command_params`` from ``lin_vel_x``, ``lin_vel_y``, ``yaw_rate`` (each a [lo, hi] pair, or a number = a fixed value),
    ``interval`` (an int or a [lo, hi] pair of control steps between draws), ``zero_prob``, ``min_lin_norm`` and ``obs_scale`` (three
    factors, default 1).  Unknown names are refused by name; what is not named takes DEFAULTS."""
    known_keys("command key", ranges, KEYS)
    r = dict(DEFAULTS, **ranges)
    p = CommandParams()
    p.seed, p.env_id_offset, p.obs_dim = int(seed) & (2 ** 64 - 1), int(env_id_offset), int(obs_dim)
    for k, name in enumerate(RANGE_KEYS):
        p.lo[k], p.hi[k] = _pair(name, r[name])
    lo, hi = (r["interval"], r["interval"]) if np.isscalar(r["interval"]) else r["interval"]
    if int(lo) != lo or int(hi) != hi or not (1 <= int(lo) <= int(hi) <= INTERVAL_MAX):
        raise ValueError("command interval must be an int or a pair of ints with 1 <= lo <= hi <= %d, got %r" % (INTERVAL_MAX, r["interval"]))
    p.interval_min, p.interval_max = int(lo), int(hi)
    p.zero_prob, p.min_lin_norm = float(r["zero_prob"]), float(r["min_lin_norm"])
    if not (0.0 <= p.zero_prob <= 1.0):
        raise ValueError("command zero_prob must lie in [0, 1], got %r" % (r["zero_prob"],))
    if not (np.isfinite(p.min_lin_norm) and p.min_lin_norm >= 0.0):
        raise ValueError("command min_lin_norm must be finite and >= 0, got %r" % (r["min_lin_norm"],))
    s = [float(v) for v in r["obs_scale"]]
    if len(s) != 3 or not all(np.isfinite(v) for v in s):
        raise ValueError("command obs_scale must be three finite factors, got %r" % (r["obs_scale"],))
    p.obs_scale[0], p.obs_scale[1], p.obs_scale[2] = s
    return p


def ranges_of(p):
    """The dict ``make_params`` would rebuild ``p`` from"""
    out = {name: (p.lo[k], p.hi[k]) for k, name in enumerate(RANGE_KEYS)}
    out.update(interval=(p.interval_min, p.interval_max), zero_prob=p.zero_prob, min_lin_norm=p.min_lin_norm, obs_scale=tuple(p.obs_scale))
    return out


def ranges_from_dict(d):
    """A command file's dict (configs/commands_walk12.yaml) -> the keyword arguments of make_params, unknown keys refused by name"""
    if not isinstance(d, dict):
        raise ValueError("a command file holds a mapping with the keys %s" % ", ".join(KEYS))
    known_keys("command key", d, KEYS)
    make_params(0, 0, 1, **d)           # (the values are checked here, by the one place that knows them)
    return dict(d)


def commands(params, mem, obs=None, out=None, cmd_out=None, restart=None, mask=None):
    """``solorl_commands``: ``params`` a CommandParams (make_params), ``mem`` a CommandMem of n rows (read and rewritten), ``obs`` float32
    [n, D] (D = params.obs_dim) or None, ``out`` float32 [n, D + 3] (default: a new tensor when ``obs`` is given; it must not overlap
    ``obs``), ``cmd_out`` float64 [n, 3] or None, ``restart`` a [n] torch.bool / torch.uint8 tensor (envs that draw now, whatever their
    countdown) or None, ``mask`` likewise (rows whose byte is 0 are neither read nor written).  -> ``out``.  One launch on the current
    stream, no host synchronisation: capturable."""
    if not isinstance(params, CommandParams) or not isinstance(mem, CommandMem):
        raise AssertionError("params must be a CommandParams and mem a CommandMem")
    d = mem.data
    n, D = d.shape[0], params.obs_dim
    if not d.is_cuda:
        raise _native.SoloRLError("commands() needs its memory rows on a GPU (there is no CPU fallback)")
    if obs is None and out is not None:
        raise AssertionError("out without obs")
    if obs is not None and out is None:
        out = torch.empty((n, D + 3), dtype=torch.float32, device=d.device)
    po = tensor_arg("obs", obs, ((n, D),), torch.float32, d.device, optional=True)
    pq = tensor_arg("out", out, ((n, D + 3),), torch.float32, d.device, optional=True)
    pc = tensor_arg("cmd_out", cmd_out, ((n, 3),), torch.float64, d.device, optional=True)
    r, pr = mask_arg(restart, n, d.device, "restart")
    m, pm = mask_arg(mask, n, d.device)
    with torch.cuda.device(d.device):
        _native.check(_native.lib().solorl_commands(C.byref(params), pm, pr, n, C.c_void_p(d.data_ptr()), po, pq, pc, torch.cuda.current_device(),
                                                    _native.stream(d.device)))
    return out
