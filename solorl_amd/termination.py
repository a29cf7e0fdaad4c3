"""Early termination rules of a whole batch: ``solorl_terminate`` (include/solorl.h, which holds the rule and row tables) from torch.

``terminate(cfg, params, states, done, reward, fired_out)`` ends the episode of every env whose state row AFTER a step breaks one of four
rules -- base too low, base tilted too far, a chosen collision primitive pressing on the ground, a joint outside its limits -- in one
kernel launch on the current stream: it sets the env's done flag, overrides its reward with the terminal reward, books the episode into
the info arrays and statistics as the engine's own fall rule does, and leaves the fired rule bits in ``fired_out``, which is the mask
``solorl_reset_masked`` takes.  ``make_termination`` builds the parameter struct from readable keys; ``SoloVecEnv.set_termination`` is the
same call behind every step.  ``rules_from_dict`` reads a termination file's dict (configs/termination_walk12.yaml).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _native
from ._native import TERM_RULES, Termination
from .config import ROBOT_SOLO12, InfoSoA, SoloConfig
from .rows import known_keys, mask_arg, state_rows, tensor_arg

RULES = ("height", "tilt", "contact", "joint")      # bit k of fired_out is RULES[k]: SOLORL_TERM_HEIGHT, _TILT, _CONTACT, _JOINT
HEIGHT, TILT, CONTACT, JOINT = 1, 2, 4, 8
STAT_FIELDS = 1 + TERM_RULES                        # term_stats [5, N]: early terminations, then how many of them each rule fired in

KEYS = ("base_height", "max_tilt_deg", "contacts", "contact_force_min", "joint_limits", "min_steps", "terminal_reward")
# primitives by group (include/solorl.h, solorl_kinematics: 0..11 base points, 12 + 2 leg knee, 13 + 2 leg foot, 20 + leg shoulder)
CONTACT_GROUPS = {"base": tuple(range(12)), "knees": (12, 14, 16, 18), "shoulders": (20, 21, 22, 23)}


def _robot(robot):
    r = robot.robot if isinstance(robot, SoloConfig) else int(robot)
    return r, (12 if r == ROBOT_SOLO12 else 8), (24 if r == ROBOT_SOLO12 else 20)


def make_termination(robot, **rules):
    """``solorl_termination`` for ``robot`` (SOLORL_ROBOT_* or a SoloConfig) from readable keys; a rule is enabled by naming its key:
      ``base_height`` [m]: the base's z below it ends the episode;
      ``max_tilt_deg``: the largest allowed angle between the base's z axis and world z (min_up_z = cos of it);
      ``contacts``: a list of group names -- ``base`` (primitives 0..11), ``knees`` (12, 14, 16, 18), ``shoulders`` (20..23, Solo12 only) --
          or explicit primitive indices; with ``contact_force_min`` [N] (default 0: any contact) the force a contact must reach;
      ``joint_limits``: one ``[lo, hi]`` pair [rad] for every joint, or one pair per joint;
    and ``min_steps`` (default 0: no rule fires before an episode's step of that number), ``terminal_reward`` (default -10, the
    engine's own).  Unknown keys are refused by name; so is a call that enables no rule."""
    known_keys("termination key", rules, KEYS)
    r, nq, nprims = _robot(robot)
    p = Termination()
    if rules.get("base_height") is not None:
        p.rules |= HEIGHT
        p.min_height = float(rules["base_height"])
    if rules.get("max_tilt_deg") is not None:
        deg = float(rules["max_tilt_deg"])
        if not (0.0 <= deg <= 180.0):
            raise ValueError("termination max_tilt_deg must lie in [0, 180], got %r" % (rules["max_tilt_deg"],))
        p.rules |= TILT
        p.min_up_z = math.cos(math.radians(deg))
    if rules.get("contacts") is not None:
        c = rules["contacts"]
        bits = 0
        for item in ([c] if isinstance(c, (str, int)) else list(c)):
            if isinstance(item, str):
                if item not in CONTACT_GROUPS:
                    raise ValueError("unknown contact group %r (known: %s, or primitive indices)" % (item, ", ".join(CONTACT_GROUPS)))
                prims = CONTACT_GROUPS[item]
            else:
                if int(item) != item:
                    raise ValueError("a contact primitive is an int or a group name, got %r" % (item,))
                prims = (int(item),)
            for q in prims:
                if not (0 <= q < nprims):
                    raise ValueError("contact primitive %d (%r) does not exist on this robot (it has 0..%d)" % (q, item, nprims - 1))
                bits |= 1 << q
        if bits == 0:
            raise ValueError("termination contacts names no primitive")
        p.rules |= CONTACT
        p.contact_prims = bits
    if rules.get("contact_force_min") is not None:
        if not (p.rules & CONTACT):
            raise ValueError("termination contact_force_min without contacts")
        p.contact_force_min = float(rules["contact_force_min"])
        if not (math.isfinite(p.contact_force_min) and p.contact_force_min >= 0.0):
            raise ValueError("termination contact_force_min must be finite and >= 0, got %r" % (rules["contact_force_min"],))
    if rules.get("joint_limits") is not None:
        lim = np.asarray(rules["joint_limits"], dtype=np.float64)
        if lim.shape == (2,):
            lim = np.broadcast_to(lim, (nq, 2))
        if lim.shape != (nq, 2) or not np.all(np.isfinite(lim)) or np.any(lim[:, 0] > lim[:, 1]):
            raise ValueError("termination joint_limits must be one finite [lo, hi] pair or %d of them with lo <= hi, got %r" % (nq, rules["joint_limits"]))
        p.rules |= JOINT
        for j in range(nq):
            p.joint_lo[j], p.joint_hi[j] = float(lim[j, 0]), float(lim[j, 1])
    if p.rules == 0:
        raise ValueError("a termination needs at least one rule (%s)" % ", ".join(KEYS[:3] + KEYS[4:5]))
    ms = rules.get("min_steps", 0)
    if int(ms) != ms or int(ms) < 0:
        raise ValueError("termination min_steps must be an int >= 0, got %r" % (ms,))
    p.min_steps = int(ms)
    p.terminal_reward = float(rules.get("terminal_reward", -10.0))
    if not math.isfinite(p.terminal_reward) or not all(math.isfinite(v) for v in (p.min_height, p.min_up_z)):
        raise ValueError("termination thresholds and terminal_reward must be finite")
    return p


def rules_from_dict(d):
    """A termination file's dict (configs/termination_walk12.yaml) -> the keyword arguments of make_termination, unknown keys refused
    by name"""
    if not isinstance(d, dict):
        raise ValueError("a termination file holds a mapping with the keys %s" % ", ".join(KEYS))
    known_keys("termination key", d, KEYS)
    return dict(d)


def terminate(cfg, params, states, done, reward, fired_out, info=None, term_stats=None, mask=None):
    """``solorl_terminate`` on the rows of ``states`` (a StateBatch on a GPU: the state AFTER the step): ``done`` uint8 [N] and ``reward``
    float32 [N] or [N, 1] of that step (rewritten where a rule fires), ``fired_out`` uint8 [N] (the rule bits that fired, 0 where none),
    ``info`` an InfoSoA of that step's arrays or None, ``term_stats`` float32 [5, N] or None (accumulated), ``mask`` a [N] torch.bool /
    torch.uint8 tensor (rows whose byte is 0 are neither read nor written).  -> ``fired_out``.  One launch on the current stream, no
    host synchronisation: capturable."""
    if not isinstance(params, Termination):
        raise AssertionError("params must be a Termination (make_termination)")
    if info is not None and not isinstance(info, InfoSoA):
        raise AssertionError("info must be an InfoSoA or None")
    d, n, dev = state_rows("terminate", cfg, states)
    pd = tensor_arg("done", done, ((n,),), torch.uint8, dev)
    pr = tensor_arg("reward", reward, ((n,), (n, 1)), torch.float32, dev)
    pf = tensor_arg("fired_out", fired_out, ((n,),), torch.uint8, dev)
    ps = tensor_arg("term_stats", term_stats, ((STAT_FIELDS, n),), torch.float32, dev, optional=True)
    m, pm = mask_arg(mask, n, dev)
    with torch.cuda.device(dev):
        _native.check(_native.lib().solorl_terminate(C.byref(cfg), C.byref(params), C.c_void_p(d.data_ptr()), pm, n, pd, pr, pf,
                                                     None if info is None else C.byref(info), ps, torch.cuda.current_device(),
                                                     _native.stream(dev)))
    return fired_out
