"""Link poses, contact points and forces of a whole batch: ``solorl_kinematics`` (include/solorl.h) from torch.

``kinematics(cfg, states)`` turns a ``StateBatch`` (what ``SoloVecEnv.get_states`` returns) into a ``KinBatch``: one float64
``[N, sizeof(solorl_env_kin) / 8]`` tensor, row i = row i of the states, with every member of ``solorl_env_kin`` as a named view --
one kernel launch on the current stream, no host synchronisation.  Every offset and shape is taken from the ctypes mirror
``EnvKin``; none is written down here.
"""
import ctypes as C
import json
import os

import numpy as np
import torch

from . import _native
from .config import SoloConfig, MAX_PRIMS, ROBOT_SOLO8, ROBOT_SOLO12
from .state import StateBatch, _shape

KIN_MAX_LINKS = 17          # SOLORL_KIN_MAX_LINKS
ENVS_PER_WORKGROUP = 18     # KIN_ENVS of csrc/solorl_kin.hip: rows one workgroup stages through LDS (a test shape, nothing else depends on it)
FOOT_PRIMS = (13, 15, 17, 19)   # the foot primitive of leg FL, FR, HL, HR (foot_prim of solorl_model_data)


class EnvKin(C.Structure):
    """ctypes mirror of ``solorl_env_kin``."""
    _fields_ = [
        ("link_pos", (C.c_double * 3) * KIN_MAX_LINKS), ("link_quat", (C.c_double * 4) * KIN_MAX_LINKS),
        ("link_com", (C.c_double * 3) * KIN_MAX_LINKS), ("link_com_vel", (C.c_double * 3) * KIN_MAX_LINKS),
        ("link_ang_vel", (C.c_double * 3) * KIN_MAX_LINKS),
        ("prim_point", (C.c_double * 3) * MAX_PRIMS), ("prim_vel", (C.c_double * 3) * MAX_PRIMS), ("prim_force", C.c_double * MAX_PRIMS),
        ("com", C.c_double * 3), ("com_vel", C.c_double * 3), ("mass", C.c_double),
        ("kinetic", C.c_double), ("potential", C.c_double), ("lin_mom", C.c_double * 3), ("ang_mom", C.c_double * 3),
    ]


ROW_BYTES = C.sizeof(EnvKin)
ROW_WORDS = ROW_BYTES // 8
assert ROW_BYTES == 3640

# member -> (byte offset, shape per row), from the ctypes structure
MEMBERS = {}
for _name, _ctype in EnvKin._fields_:
    _s, _base = _shape(_ctype)
    assert _base is C.c_double, _name
    MEMBERS[_name] = (getattr(EnvKin, _name).offset, _s)


def _link_names(robot):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "models", "solo12.json" if robot == ROBOT_SOLO12 else "solo8.json")
    with open(path) as f:
        return tuple(l["name"] for l in json.load(f)["links"])


# link order of solorl_model_data = row order of the link_* members
LINK_NAMES = {ROBOT_SOLO8: _link_names(ROBOT_SOLO8), ROBOT_SOLO12: _link_names(ROBOT_SOLO12)}


class KinBatch:
    """``data``: float64 ``[N, ROW_WORDS]`` (contiguous).  Views named after the members of ``solorl_env_kin``: ``link_pos [N,17,3]``,
    ``link_quat [N,17,4]`` (x y z w), ``link_com``, ``link_com_vel``, ``link_ang_vel [N,17,3]``, ``prim_point [N,24,3]``, ``prim_vel``,
    ``prim_force [N,24]``, ``com [N,3]``, ``com_vel``, ``mass [N]``, ``kinetic``, ``potential``, ``lin_mom [N,3]``, ``ang_mom``; and over
    the feet's primitives (legs FL, FR, HL, HR) ``foot_pos [N,4,3]``, ``foot_vel [N,4,3]``, ``foot_force [N,4]``."""

    def __init__(self, num_envs=None, device=None, data=None):
        if data is None:
            data = torch.zeros((int(num_envs), ROW_WORDS), dtype=torch.float64, device=device)
        if not (data.dtype == torch.float64 and data.dim() == 2 and data.shape[1] == ROW_WORDS and data.is_contiguous()):
            raise AssertionError("KinBatch data must be a contiguous float64 [N, %d] tensor" % ROW_WORDS)
        self.data = data
        for name, (off, shape) in MEMBERS.items():
            n = int(np.prod(shape)) if shape else 1
            v = data[:, off // 8: off // 8 + n]
            setattr(self, name, v.unflatten(1, shape) if len(shape) > 1 else (v if shape else v[:, 0]))
        self.foot_pos = self.prim_point[:, FOOT_PRIMS[0]:FOOT_PRIMS[-1] + 1:2]
        self.foot_vel = self.prim_vel[:, FOOT_PRIMS[0]:FOOT_PRIMS[-1] + 1:2]
        self.foot_force = self.prim_force[:, FOOT_PRIMS[0]:FOOT_PRIMS[-1] + 1:2]

    @property
    def num_envs(self):
        return self.data.shape[0]

    @property
    def device(self):
        return self.data.device

    def clone(self):
        return KinBatch(data=self.data.clone())

    def bytes(self):
        """uint8 [N, ROW_BYTES] view, for bitwise comparisons"""
        return self.data.view(torch.uint8)


def kinematics(cfg, states, mask=None, out=None):
    """``solorl_kinematics`` on the rows of ``states`` (a StateBatch on a GPU) -> ``KinBatch`` on the same device.  ``cfg``: a
    SoloConfig; its robot, use_urdf_inertia, sim_dt and gravity are read.  ``mask``: a [N] torch.bool / torch.uint8 tensor; rows whose
    byte is 0 are neither read nor written (zeros in a fresh ``out``).  Enqueued on the current stream; capturable."""
    if not isinstance(cfg, SoloConfig):
        raise AssertionError("cfg must be a SoloConfig")
    if not isinstance(states, StateBatch):
        raise AssertionError("states must be a StateBatch")
    d = states.data
    n = d.shape[0]
    if not d.is_cuda:
        raise _native.SoloRLError("kinematics() needs state rows on a GPU (there is no CPU fallback)")
    if out is None:
        out = KinBatch(n, d.device)
    if not (isinstance(out, KinBatch) and out.data.device == d.device and out.data.shape[0] == n):
        raise AssertionError("out must be a KinBatch of %d rows on %s" % (n, d.device))
    pm = C.c_void_p(0)
    if mask is not None:
        if not (mask.is_cuda and mask.device == d.device and mask.dtype in (torch.bool, torch.uint8) and mask.is_contiguous()
                and tuple(mask.shape) == (n,)):
            raise AssertionError("mask must be a contiguous torch.bool or torch.uint8 [%d] tensor on %s" % (n, d.device))
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        pm = C.c_void_p(mask.data_ptr())
    with torch.cuda.device(d.device):
        _native.check(_native.lib().solorl_kinematics(C.byref(cfg), C.c_void_p(d.data_ptr()), pm, n, C.c_void_p(out.data.data_ptr()),
                                                      torch.cuda.current_device(), _native.stream(d.device)))
    return out
