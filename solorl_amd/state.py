"""The state of a whole batch of envs as ONE tensor: ``[N, sizeof(solorl_env_state) / 8]`` float64, row i = env i, the
array ``solorl_get_states`` / ``solorl_set_states`` (include/solorl.h) read and write on the device.

``StateBatch`` owns that tensor and exposes every member of ``solorl_env_state`` as a named, writable view of it.  Every
offset and shape is taken from the ctypes mirror ``EnvState`` (config.py); none is written down here.
"""
import ctypes as C

import numpy as np
import torch

from .config import EnvState

ROW_BYTES = C.sizeof(EnvState)
ROW_WORDS = ROW_BYTES // 8
assert ROW_BYTES % 8 == 0

# SOLORL_SF_* (include/solorl.h): the member groups solorl_set_states writes
SF_POSE, SF_VEL, SF_JOINT_POS, SF_JOINT_VEL, SF_CONTACT, SF_HISTORY, SF_TASK, SF_COUNTERS, SF_ALL = 1, 2, 4, 8, 16, 32, 64, 128, 255
FIELD_BITS = {"pose": SF_POSE, "vel": SF_VEL, "joint_pos": SF_JOINT_POS, "joint_vel": SF_JOINT_VEL, "contact": SF_CONTACT,
              "history": SF_HISTORY, "task": SF_TASK, "counters": SF_COUNTERS, "all": SF_ALL}
# which group each member belongs to (tau belongs to none: it reads 0 and is ignored on write)
GROUP_MEMBERS = {"pose": ("pos", "quat"), "vel": ("lin_vel", "ang_vel"), "joint_pos": ("q",), "joint_vel": ("qd",),
                 "contact": ("lambda_prev", "contact_mask"), "history": ("hist",),
                 "task": ("goal", "potential", "progress", "goals_reached", "env_goals_reached", "dr", "treadmill_y"),
                 "counters": ("timestep", "need_reset", "rng_counter")}


def field_bits(fields):
    """A group name, an iterable of names, or an int of SOLORL_SF_* bits -> the int."""
    if isinstance(fields, str):
        fields = (fields,)
    if isinstance(fields, int):
        return fields
    bits = 0
    for f in fields:
        if f not in FIELD_BITS:
            raise ValueError("unknown state field group %r (one of %s)" % (f, ", ".join(sorted(FIELD_BITS))))
        bits |= FIELD_BITS[f]
    return bits


def _shape(ctype):
    s = []
    while hasattr(ctype, "_length_"):
        s.append(ctype._length_)
        ctype = ctype._type_
    return tuple(s), ctype


# member -> (byte offset, shape per env, is int32), from the ctypes structure
MEMBERS = {}
for _name, _ctype in EnvState._fields_:
    _s, _base = _shape(_ctype)
    assert _base in (C.c_double, C.c_int32), _name
    MEMBERS[_name] = (getattr(EnvState, _name).offset, _s, _base is C.c_int32)


class StateBatch:
    """``data``: float64 ``[N, ROW_WORDS]`` (contiguous).  Attributes named after the members of ``solorl_env_state`` are views of it:
    ``pos [N,3]``, ``quat [N,4]``, ``lin_vel``, ``ang_vel``, ``q [N,12]``, ``qd``, ``tau``, ``lambda_prev [N,24]``, ``hist [N,4,42]``,
    ``goal [N,2]``, ``potential [N]``, ``progress``, ``goals_reached``, ``env_goals_reached``, ``dr [N,5]``, ``treadmill_y`` (float64) and
    ``timestep [N]``, ``need_reset``, ``contact_mask``, ``rng_counter`` (int32).  Writing through a view writes the row array."""

    def __init__(self, num_envs=None, device=None, data=None):
        if data is None:
            data = torch.zeros((int(num_envs), ROW_WORDS), dtype=torch.float64, device=device)
        if not (data.dtype == torch.float64 and data.dim() == 2 and data.shape[1] == ROW_WORDS and data.is_contiguous()):
            raise AssertionError("StateBatch data must be a contiguous float64 [N, %d] tensor" % ROW_WORDS)
        self.data = data
        ints = data.view(torch.int32)                      # [N, 2 * ROW_WORDS]
        for name, (off, shape, is_int) in MEMBERS.items():
            if is_int:
                v = ints[:, off // 4]
            else:
                n = int(np.prod(shape)) if shape else 1
                v = data[:, off // 8: off // 8 + n]
                v = v.unflatten(1, shape) if len(shape) > 1 else (v if shape else v[:, 0])
            setattr(self, name, v)

    @property
    def num_envs(self):
        return self.data.shape[0]

    @property
    def device(self):
        return self.data.device

    def clone(self):
        return StateBatch(data=self.data.clone())

    def bytes(self):
        """uint8 [N, ROW_BYTES] view: for bitwise comparisons (NaN patterns and the integer members included)"""
        return self.data.view(torch.uint8)

    def env_state(self, i):
        """Row i as a host ``EnvState`` (what the oracle's and the engine's per-env ``set_state`` take)."""
        row = self.data[int(i)].detach().cpu().contiguous().view(torch.uint8).numpy()
        return EnvState.from_buffer_copy(row.tobytes())

    @classmethod
    def from_env_states(cls, states, device=None):
        """A batch from a sequence of host ``EnvState`` rows (bytes are copied as they are)."""
        raw = np.frombuffer(b"".join(bytes(s) for s in states), dtype=np.uint8).reshape(len(states), ROW_BYTES).copy()
        t = torch.from_numpy(raw)
        if device is not None:
            t = t.to(device)
        return cls(data=t.view(torch.float64))
