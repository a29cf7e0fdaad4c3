"""Link poses, contact points and forces of a whole batch: ``solorl_kinematics`` (include/solorl.h) from torch.

``kinematics(cfg, states)`` turns a ``StateBatch`` (what ``SoloVecEnv.get_states`` returns) into a ``KinBatch``: one float64
``[N, sizeof(solorl_env_kin) / 8]`` tensor, row i = row i of the states, with every member of ``solorl_env_kin`` as a named view --
one kernel launch on the current stream, no host synchronisation.  Every offset and shape is taken from the ctypes mirror
``EnvKin``; none is written down here.
"""
import ctypes as C
import json
import os

from .config import MAX_PRIMS, ROBOT_SOLO8, ROBOT_SOLO12
from .rows import RowBatch, call_rows, members_of

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
MEMBERS = members_of(EnvKin)


def _link_names(robot):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "models", "solo12.json" if robot == ROBOT_SOLO12 else "solo8.json")
    with open(path) as f:
        return tuple(l["name"] for l in json.load(f)["links"])


# link order of solorl_model_data = row order of the link_* members
LINK_NAMES = {ROBOT_SOLO8: _link_names(ROBOT_SOLO8), ROBOT_SOLO12: _link_names(ROBOT_SOLO12)}


class KinBatch(RowBatch):
    """``data``: float64 ``[N, ROW_WORDS]`` (contiguous).  Views named after the members of ``solorl_env_kin``: ``link_pos [N,17,3]``,
    ``link_quat [N,17,4]`` (x y z w), ``link_com``, ``link_com_vel``, ``link_ang_vel [N,17,3]``, ``prim_point [N,24,3]``, ``prim_vel``,
    ``prim_force [N,24]``, ``com [N,3]``, ``com_vel``, ``mass [N]``, ``kinetic``, ``potential``, ``lin_mom [N,3]``, ``ang_mom``; and over
    the feet's primitives (legs FL, FR, HL, HR) ``foot_pos [N,4,3]``, ``foot_vel [N,4,3]``, ``foot_force [N,4]``."""
    MIRROR = EnvKin

    def __init__(self, num_envs=None, device=None, data=None):
        super().__init__(num_envs, device, data)
        self.foot_pos = self.prim_point[:, FOOT_PRIMS[0]:FOOT_PRIMS[-1] + 1:2]
        self.foot_vel = self.prim_vel[:, FOOT_PRIMS[0]:FOOT_PRIMS[-1] + 1:2]
        self.foot_force = self.prim_force[:, FOOT_PRIMS[0]:FOOT_PRIMS[-1] + 1:2]


def kinematics(cfg, states, mask=None, out=None):
    """``solorl_kinematics`` on the rows of ``states`` (a StateBatch on a GPU) -> ``KinBatch`` on the same device.  ``cfg``: a
    SoloConfig; its robot, use_urdf_inertia, sim_dt and gravity are read.  ``mask``: a [N] torch.bool / torch.uint8 tensor; rows whose
    byte is 0 are neither read nor written (zeros in a fresh ``out``).  Enqueued on the current stream; capturable."""
    return call_rows("kinematics", cfg, states, KinBatch, mask, out)
