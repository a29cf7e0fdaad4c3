"""Randomised initial states of a whole batch: ``solorl_randomize_reset`` and ``solorl_restart_history`` (include/solorl.h, which holds
the draw table) from torch.

``randomize_reset(cfg, params, states, count)`` changes the rows of a StateBatch in place, in one kernel launch on the current stream:
joint angles and velocities, base velocity, heading, roll and pitch get a uniform offset drawn from a Philox stream per env and episode,
and -- with ``place_on_ground`` -- the robot is moved up or down until the lowest support point of its collision primitives lies
``clearance`` above the ground.  ``make_reset_randomization`` builds the parameter struct from readable keys; ``ranges_from_dict`` reads
a file's dict (configs/reset_walk12.yaml).  ``SoloVecEnv.set_reset_randomization`` is the chain get_states -> randomize_reset ->
set_states -> restart_history behind every reset.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _native
from ._native import ResetRandomization
from .config import ROBOT_SOLO12, SoloConfig
from .rows import known_keys, mask_arg, state_rows, tensor_arg

ENVS_PER_WORKGROUP = 64     # RESET_ENVS of csrc/solorl_reset.hip
KEYS = ("joint_pos", "joint_vel", "lin_vel", "ang_vel", "yaw", "roll", "pitch", "clearance", "place_on_ground")


def _widths(name, x, n, full):
    """a scalar or an n-sequence of half-widths -> ``full`` doubles (the rest 0), each finite and >= 0"""
    v = np.asarray(x, dtype=np.float64)
    if v.ndim == 0:
        v = np.full((n,), float(v))
    if v.shape != (n,) or not np.all(np.isfinite(v)) or np.any(v < 0):
        raise ValueError("reset randomization %s must be one finite half-width >= 0 or %d of them, got %r" % (name, n, x))
    return (C.c_double * full)(*(v.tolist() + [0.0] * (full - n)))


def make_reset_randomization(cfg, seed, id0, **ranges):
    """``solorl_reset_randomization`` for ``cfg``'s robot, keyed by ``seed`` and the global env id ``id0 + i``, from half-widths:
      ``joint_pos`` [rad], ``joint_vel`` [rad/s]: a scalar or one value per joint; q is clamped to +-cfg.joint_limit afterwards;
      ``lin_vel`` [m/s], ``ang_vel`` [rad/s]: a scalar or (x, y, z), world frame;
      ``yaw``, ``roll``, ``pitch`` [rad], each <= pi: yaw about the world's z axis, roll and pitch about the body's x and y axes;
      ``place_on_ground`` (default True) with ``clearance`` [m] (default 0): the base height is changed until the lowest support point
      of the robot's collision primitives lies ``clearance`` above z = 0.
    Everything defaults to 0 (an exact no-op for that member).  Unknown keys are refused by name."""
    known_keys("reset randomization key", ranges, KEYS)
    if not isinstance(cfg, SoloConfig):
        raise AssertionError("cfg must be a SoloConfig")
    nq = 12 if cfg.robot == ROBOT_SOLO12 else 8
    p = ResetRandomization()
    p.seed, p.env_id_offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(id0)
    p.joint_pos = _widths("joint_pos", ranges.get("joint_pos", 0.0), nq, 12)
    p.joint_vel = _widths("joint_vel", ranges.get("joint_vel", 0.0), nq, 12)
    p.lin_vel = _widths("lin_vel", ranges.get("lin_vel", 0.0), 3, 3)
    p.ang_vel = _widths("ang_vel", ranges.get("ang_vel", 0.0), 3, 3)
    for name in ("yaw", "roll", "pitch"):
        a = float(ranges.get(name, 0.0))
        if not (math.isfinite(a) and 0.0 <= a <= math.pi):
            raise ValueError("reset randomization %s must lie in [0, pi], got %r" % (name, ranges.get(name)))
        setattr(p, name, a)
    p.clearance = float(ranges.get("clearance", 0.0))
    if not (math.isfinite(p.clearance) and p.clearance >= 0.0):
        raise ValueError("reset randomization clearance must be finite and >= 0, got %r" % (ranges.get("clearance"),))
    p.place_on_ground = 1 if ranges.get("place_on_ground", True) else 0
    return p


def ranges_from_dict(d):
    """A reset-randomization file's dict (configs/reset_walk12.yaml) -> the keyword arguments of make_reset_randomization, unknown keys
    refused by name"""
    if not isinstance(d, dict):
        raise ValueError("a reset randomization file holds a mapping with the keys %s" % ", ".join(KEYS))
    known_keys("reset randomization key", d, KEYS)
    return dict(d)


def randomize_reset(cfg, params, states, count, mask=None):
    """``solorl_randomize_reset`` on the rows of ``states`` (a StateBatch on a GPU), in place: ``count`` int32 [N] (uint32 words: each
    selected env's episode index, advanced by one), ``mask`` a [N] torch.bool / torch.uint8 tensor (rows whose byte is 0 and their
    count are neither read nor written).  -> ``states``.  One launch on the current stream, no host synchronisation: capturable."""
    if not isinstance(params, ResetRandomization):
        raise AssertionError("params must be a ResetRandomization (make_reset_randomization)")
    d, n, dev = state_rows("randomize_reset", cfg, states)
    pc = tensor_arg("count", count, ((n,),), torch.int32, dev)
    m, pm = mask_arg(mask, n, dev)
    with torch.cuda.device(dev):
        _native.check(_native.lib().solorl_randomize_reset(C.byref(cfg), C.byref(params), C.c_void_p(d.data_ptr()), pm, pc, n,
                                                           torch.cuda.current_device(), _native.stream(dev)))
    return states
