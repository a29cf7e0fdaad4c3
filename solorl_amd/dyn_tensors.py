"""Mass matrix, bias and gravity forces and foot Jacobians of a whole batch: ``solorl_dynamics`` (include/solorl.h) from torch.

``dynamics(cfg, states)`` turns a ``StateBatch`` (what ``SoloVecEnv.get_states`` returns) into a ``DynBatch``: one float64
``[N, sizeof(solorl_env_dyn) / 8]`` tensor, row i = row i of the states, with every member of ``solorl_env_dyn`` as a named view --
one kernel launch on the current stream, no host synchronisation.  Every offset and shape is taken from the ctypes mirror
``EnvDyn``; none is written down here.  Conventions (generalised velocity ``[lin_vel, ang_vel, qd]``, Solo8 padding, the oracle's
order): the comment above ``solorl_env_dyn`` in the header.
"""
import ctypes as C

import torch

from .rows import RowBatch, call_rows, members_of

NV = 18                     # SOLORL_DYN_NV: 6 base coordinates + 12 joints (a Solo8 uses 14; the rest reads 0)
ENVS_PER_WORKGROUP = 16     # DYN_ENVS of csrc/solorl_dyn.hip: rows one workgroup stages through LDS (a test shape, nothing else depends on it)


class EnvDyn(C.Structure):
    """ctypes mirror of ``solorl_env_dyn``."""
    _fields_ = [
        ("mass_matrix", (C.c_double * NV) * NV), ("bias", C.c_double * NV), ("gravity", C.c_double * NV),
        ("foot_jac", ((C.c_double * NV) * 3) * 4), ("foot_acc_bias", (C.c_double * 3) * 4), ("foot_pos", (C.c_double * 3) * 4),
    ]


ROW_BYTES = C.sizeof(EnvDyn)
ROW_WORDS = ROW_BYTES // 8
assert ROW_BYTES == 4800 and ROW_WORDS == 600

# member -> (byte offset, shape per row), from the ctypes structure
MEMBERS = members_of(EnvDyn)


class DynBatch(RowBatch):
    """``data``: float64 ``[N, ROW_WORDS]`` (contiguous).  Views named after the members of ``solorl_env_dyn``: ``mass_matrix [N,18,18]``,
    ``bias [N,18]``, ``gravity [N,18]``, ``foot_jac [N,4,3,18]``, ``foot_acc_bias [N,4,3]``, ``foot_pos [N,4,3]`` (legs FL, FR, HL, HR)."""
    MIRROR = EnvDyn


def velocity(states):
    """The generalised velocity ``[N, 18]`` the tensors are written for: ``lin_vel``, ``ang_vel``, ``qd`` of a StateBatch, in that order."""
    return torch.cat((states.lin_vel, states.ang_vel, states.qd), dim=1)


def dynamics(cfg, states, mask=None, out=None):
    """``solorl_dynamics`` on the rows of ``states`` (a StateBatch on a GPU) -> ``DynBatch`` on the same device.  ``cfg``: a
    SoloConfig; its robot, use_urdf_inertia, gravity and damping are read.  ``mask``: a [N] torch.bool / torch.uint8 tensor; rows whose
    byte is 0 are neither read nor written (zeros in a fresh ``out``).  Enqueued on the current stream; capturable."""
    return call_rows("dynamics", cfg, states, DynBatch, mask, out)
