"""Mass matrix, bias and gravity forces and foot Jacobians of a whole batch: ``solorl_dynamics`` (include/solorl.h) from torch.

``dynamics(cfg, states)`` turns a ``StateBatch`` (what ``SoloVecEnv.get_states`` returns) into a ``DynBatch``: one float64
``[N, sizeof(solorl_env_dyn) / 8]`` tensor, row i = row i of the states, with every member of ``solorl_env_dyn`` as a named view --
one kernel launch on the current stream, no host synchronisation.  Every offset and shape is taken from the ctypes mirror
``EnvDyn``; none is written down here.  Conventions (generalised velocity ``[lin_vel, ang_vel, qd]``, Solo8 padding, the oracle's
order): the comment above ``solorl_env_dyn`` in the header.
"""
import ctypes as C

import numpy as np
import torch

from . import _native
from .config import SoloConfig
from .state import StateBatch, _shape

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
MEMBERS = {}
for _name, _ctype in EnvDyn._fields_:
    _s, _base = _shape(_ctype)
    assert _base is C.c_double, _name
    MEMBERS[_name] = (getattr(EnvDyn, _name).offset, _s)


class DynBatch:
    """``data``: float64 ``[N, ROW_WORDS]`` (contiguous).  Views named after the members of ``solorl_env_dyn``: ``mass_matrix [N,18,18]``,
    ``bias [N,18]``, ``gravity [N,18]``, ``foot_jac [N,4,3,18]``, ``foot_acc_bias [N,4,3]``, ``foot_pos [N,4,3]`` (legs FL, FR, HL, HR)."""

    def __init__(self, num_envs=None, device=None, data=None):
        if data is None:
            data = torch.zeros((int(num_envs), ROW_WORDS), dtype=torch.float64, device=device)
        if not (data.dtype == torch.float64 and data.dim() == 2 and data.shape[1] == ROW_WORDS and data.is_contiguous()):
            raise AssertionError("DynBatch data must be a contiguous float64 [N, %d] tensor" % ROW_WORDS)
        self.data = data
        for name, (off, shape) in MEMBERS.items():
            n = int(np.prod(shape))
            v = data[:, off // 8: off // 8 + n]
            setattr(self, name, v.unflatten(1, shape) if len(shape) > 1 else v)

    @property
    def num_envs(self):
        return self.data.shape[0]

    @property
    def device(self):
        return self.data.device

    def clone(self):
        return DynBatch(data=self.data.clone())

    def bytes(self):
        """uint8 [N, ROW_BYTES] view, for bitwise comparisons"""
        return self.data.view(torch.uint8)


def velocity(states):
    """The generalised velocity ``[N, 18]`` the tensors are written for: ``lin_vel``, ``ang_vel``, ``qd`` of a StateBatch, in that order."""
    return torch.cat((states.lin_vel, states.ang_vel, states.qd), dim=1)


def dynamics(cfg, states, mask=None, out=None):
    """``solorl_dynamics`` on the rows of ``states`` (a StateBatch on a GPU) -> ``DynBatch`` on the same device.  ``cfg``: a
    SoloConfig; its robot, use_urdf_inertia, gravity and damping are read.  ``mask``: a [N] torch.bool / torch.uint8 tensor; rows whose
    byte is 0 are neither read nor written (zeros in a fresh ``out``).  Enqueued on the current stream; capturable."""
    if not isinstance(cfg, SoloConfig):
        raise AssertionError("cfg must be a SoloConfig")
    if not isinstance(states, StateBatch):
        raise AssertionError("states must be a StateBatch")
    d = states.data
    n = d.shape[0]
    if not d.is_cuda:
        raise _native.SoloRLError("dynamics() needs state rows on a GPU (there is no CPU fallback)")
    if out is None:
        out = DynBatch(n, d.device)
    if not (isinstance(out, DynBatch) and out.data.device == d.device and out.data.shape[0] == n):
        raise AssertionError("out must be a DynBatch of %d rows on %s" % (n, d.device))
    pm = C.c_void_p(0)
    if mask is not None:
        if not (mask.is_cuda and mask.device == d.device and mask.dtype in (torch.bool, torch.uint8) and mask.is_contiguous()
                and tuple(mask.shape) == (n,)):
            raise AssertionError("mask must be a contiguous torch.bool or torch.uint8 [%d] tensor on %s" % (n, d.device))
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        pm = C.c_void_p(mask.data_ptr())
    with torch.cuda.device(d.device):
        _native.check(_native.lib().solorl_dynamics(C.byref(cfg), C.c_void_p(d.data_ptr()), pm, n, C.c_void_p(out.data.data_ptr()),
                                                    torch.cuda.current_device(), _native.stream(d.device)))
    return out
