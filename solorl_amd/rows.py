"""Batches of rows and the calls that turn state rows into derived rows (include/solorl.h solorl_kinematics, solorl_dynamics).

A batch is ONE ``[N, sizeof(struct) / word size]`` tensor of float64 (or float32) words, row i = env i, with every member of the C struct as
a named view of it.  ``RowBatch`` is that, for any ctypes mirror; ``StateBatch`` is the batch of ``solorl_env_state`` (solorl_amd/state.py
describes its member groups), ``KinBatch`` and ``DynBatch`` (kinematics.py, dyn_tensors.py) the two derived ones, ``ShapeMem``,
``CommandMem`` and ``ActuatorMem`` (shaping.py, command.py, channel.py) the per-env memories.  Every offset and shape is taken from the
mirrors; none is written down.  ``call_rows`` is the one call behind ``kinematics()`` and ``dynamics()``.

What every wrapper of a handle-free entry point shares is here too: ``tensor_arg`` (the one check of an argument that goes to the C ABI as
a raw pointer), ``mask_arg``, ``state_rows`` (the front matter of a call on state rows) and ``known_keys`` (the one refusal of an unknown
key).
"""
import ctypes as C
import functools

import numpy as np
import torch

from . import _native
from .config import EnvState, SoloConfig


def _shape(ctype):
    s = []
    while hasattr(ctype, "_length_"):
        s.append(ctype._length_)
        ctype = ctype._type_
    return tuple(s), ctype


_INTS = (C.c_int32, C.c_uint32)


@functools.lru_cache(maxsize=None)
def members_of(struct, int32=False, word=C.c_double):
    """member -> (byte offset, shape per row) of a ctypes mirror made of ``word`` members; with ``int32`` its members may be (u)int32 too
    and the values are (byte offset, shape per row, is int32)"""
    out = {}
    for name, ctype in struct._fields_:
        s, base = _shape(ctype)
        assert base is word or (int32 and base in _INTS), name
        out[name] = (getattr(struct, name).offset, s) + ((base in _INTS,) if int32 else ())
    return out


def tensor_arg(name, x, shapes, dtype, device, optional=False):
    """The one check of an argument the C ABI takes as a raw pointer: ``x`` must be a tensor on ``device`` (same index), of ``dtype``,
    contiguous, of one of ``shapes`` -> its pointer; with ``optional``, None -> a null pointer"""
    if x is None and optional:
        return C.c_void_p(0)
    if not (isinstance(x, torch.Tensor) and x.device == device and x.dtype == dtype and x.is_contiguous() and tuple(x.shape) in shapes):
        got = ("%s %s%s on %s" % (x.dtype, tuple(x.shape), "" if x.is_contiguous() else " (not contiguous)", x.device)
               if isinstance(x, torch.Tensor) else "None" if x is None else "a %s" % type(x).__name__)
        raise AssertionError("%s must be a contiguous %s %s tensor on %s, got %s" % (
            name, str(dtype).replace("torch.", ""), " or ".join(str(list(sh)) for sh in shapes), device, got))
    return C.c_void_p(x.data_ptr())


def known_keys(what, given, known):
    """Refuses by name what ``given`` holds beyond ``known``"""
    unknown = sorted(set(given) - set(known))
    if unknown:
        raise ValueError("unknown %s(s) %s (known: %s)" % (what, ", ".join(map(repr, unknown)), ", ".join(known)))


class RowBatch:
    """``data``: ``[N, sizeof(MIRROR) / word size]`` of ``WORD`` (float64 or float32, contiguous).  Attributes named after the members of
    the ctypes mirror ``MIRROR`` (both set by the subclass) are views of it -- its (u)int32 members as int32 views; writing through a view
    writes the row array."""
    MIRROR = None
    WORD = torch.float64

    def __init__(self, num_envs=None, device=None, data=None):
        size, ctype = (8, C.c_double) if self.WORD == torch.float64 else (4, C.c_float)
        words = C.sizeof(self.MIRROR) // size
        if data is None:
            data = torch.zeros((int(num_envs), words), dtype=self.WORD, device=device)
        if not (data.dtype == self.WORD and data.dim() == 2 and data.shape[1] == words and data.is_contiguous()):
            raise AssertionError("%s data must be a contiguous %s [N, %d] tensor" % (type(self).__name__, str(self.WORD).replace("torch.", ""), words))
        self.data = data
        ints = data.view(torch.int32)
        for name, (off, shape, is_int) in members_of(self.MIRROR, True, ctype).items():
            if is_int:
                setattr(self, name, ints[:, off // 4])
            else:
                n = int(np.prod(shape)) if shape else 1
                v = data[:, off // size: off // size + n]
                setattr(self, name, v.unflatten(1, shape) if len(shape) > 1 else (v if shape else v[:, 0]))

    @property
    def num_envs(self):
        return self.data.shape[0]

    @property
    def device(self):
        return self.data.device

    def clone(self):
        return type(self)(data=self.data.clone())

    def bytes(self):
        """uint8 [N, row bytes] view: for bitwise comparisons (NaN patterns and integer members included)"""
        return self.data.view(torch.uint8)


class StateBatch(RowBatch):
    """``data``: float64 ``[N, ROW_WORDS]`` (contiguous).  Attributes named after the members of ``solorl_env_state`` are views of it:
    ``pos [N,3]``, ``quat [N,4]``, ``lin_vel``, ``ang_vel``, ``q [N,12]``, ``qd``, ``tau``, ``lambda_prev [N,24]``, ``hist [N,4,42]``,
    ``goal [N,2]``, ``potential [N]``, ``progress``, ``goals_reached``, ``env_goals_reached``, ``dr [N,5]``, ``treadmill_y`` (float64) and
    ``timestep [N]``, ``need_reset``, ``contact_mask``, ``rng_counter`` (int32).  Writing through a view writes the row array."""
    MIRROR = EnvState

    def env_state(self, i):
        """Row i as a host ``EnvState`` (what the oracle's and the engine's per-env ``set_state`` take)."""
        row = self.data[int(i)].detach().cpu().contiguous().view(torch.uint8).numpy()
        return EnvState.from_buffer_copy(row.tobytes())

    @classmethod
    def from_env_states(cls, states, device=None):
        """A batch from a sequence of host ``EnvState`` rows (bytes are copied as they are)."""
        raw = np.frombuffer(b"".join(bytes(s) for s in states), dtype=np.uint8).reshape(len(states), C.sizeof(EnvState)).copy()
        t = torch.from_numpy(raw)
        if device is not None:
            t = t.to(device)
        return cls(data=t.view(torch.float64))


def mask_arg(mask, n, device, name="mask"):
    """None, or a [n] torch.bool / torch.uint8 tensor on ``device`` -> (tensor kept alive for the call, pointer)"""
    if mask is None:
        return None, C.c_void_p(0)
    if not (mask.is_cuda and mask.device == device and mask.dtype in (torch.bool, torch.uint8) and mask.is_contiguous()
            and tuple(mask.shape) == (n,)):
        raise AssertionError("%s must be a contiguous torch.bool or torch.uint8 [%d] tensor on %s" % (name, n, device))
    m = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    return m, C.c_void_p(m.data_ptr())


def state_rows(fn, cfg, states):
    """The front matter of a row query ``fn``: ``cfg`` a SoloConfig, ``states`` a StateBatch on a GPU -> (its data, rows, device)"""
    if not isinstance(cfg, SoloConfig):
        raise AssertionError("cfg must be a SoloConfig")
    if not isinstance(states, StateBatch):
        raise AssertionError("states must be a StateBatch")
    d = states.data
    if not d.is_cuda:
        raise _native.SoloRLError("%s() needs state rows on a GPU (there is no CPU fallback)" % fn)
    return d, d.shape[0], d.device


def call_rows(entry, cfg, states, batch_cls, mask=None, out=None):
    """``solorl_<entry>`` on the rows of ``states`` (a StateBatch on a GPU) -> ``batch_cls`` on the same device: one kernel launch on
    the current stream, no host synchronisation."""
    d, n, _ = state_rows(entry, cfg, states)
    if out is None:
        out = batch_cls(n, d.device)
    if not (isinstance(out, batch_cls) and out.data.device == d.device and out.data.shape[0] == n):
        raise AssertionError("out must be a %s of %d rows on %s" % (batch_cls.__name__, n, d.device))
    m, pm = mask_arg(mask, n, d.device)
    with torch.cuda.device(d.device):
        _native.check(getattr(_native.lib(), "solorl_" + entry)(C.byref(cfg), C.c_void_p(d.data_ptr()), pm, n, C.c_void_p(out.data.data_ptr()),
                                                                torch.cuda.current_device(), _native.stream(d.device)))
    return out
