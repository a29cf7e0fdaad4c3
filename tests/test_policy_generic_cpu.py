"""The width-generic policy kernels' entry points (include/solorl.h: solorl_policy_act_w, solorl_ppo_grad_stage1_w / stage2_w,
solorl_ppo_clip_adam_w) and their Python switch, as far as a machine without a GPU can see them: every refusal precedes the device
lookup, a shape inside the cap gets as far as that lookup, and with the switch unset nothing chooses the family."""
import ctypes as C

import numpy as np
import pytest
import torch

from solorl_amd import _native, build


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


def _tables(obs_dim, act_dim, hidden=64, critic_obs_dim=0):
    P = _native.PolicyParams()
    P.obs_dim, P.act_dim, P.hidden, P.critic_obs_dim = obs_dim, act_dim, hidden, critic_obs_dim
    for k, _t in P._fields_[4:]:
        setattr(P, k, 4096)                           # non-null, 16-byte aligned (never dereferenced on the host)
    B, W, G, S = _native.PpoBatch(), _native.PpoStage1(), _native.PpoGrads(), _native.AdamState()
    for st in (B, W, G, S):
        for k, t in st._fields_:
            if t is C.c_void_p:
                setattr(st, k, 4096)
    B.m = 64
    return P, B, W, G, S


def _calls(lib, P, B, W, G, S, critic):
    """the four entry points on dummy arrays; critic: whether the critic's arrays are given"""
    d = C.c_void_p(4096)
    c = d if critic else None
    return {"solorl_policy_act_w": lambda: lib.solorl_policy_act_w(C.byref(P), d, c, None, 64, d, d, d, 0, None),
            "solorl_ppo_grad_stage1_w": lambda: lib.solorl_ppo_grad_stage1_w(C.byref(P), C.byref(B), c, C.byref(W), c, 0, None),
            "solorl_ppo_grad_stage2_w": lambda: lib.solorl_ppo_grad_stage2_w(C.byref(P), C.byref(W), c, 64, C.byref(G), 0, None),
            "solorl_ppo_clip_adam_w": lambda: lib.solorl_ppo_clip_adam_w(C.byref(P), C.byref(G), C.byref(S), 0, None)}


def test_the_cap_is_the_headers(lib):
    hdr = open(build.INC[0]).read()
    assert "#define SOLORL_POLICY_MAX_WIDTH %d\n" % _native.POLICY_MAX_WIDTH in hdr and _native.POLICY_MAX_WIDTH == 128


@pytest.mark.parametrize("obs,critic,act,hidden", [(129, 0, 12, 64), (76, 129, 12, 64), (76, 0, 16, 64), (76, 0, 12, 32), (76, 76, 12, 64),
                                                   (0, 0, 12, 64), (76, -4, 8, 64)])
def test_entry_points_refuse_shapes_outside_the_family_and_name_the_cap(lib, obs, critic, act, hidden):
    P, B, W, G, S = _tables(obs, act, hidden, critic)
    for name, call in _calls(lib, P, B, W, G, S, critic != 0).items():
        assert call() == -1, name                     # SOLORL_ERR_INVALID
        msg = lib.solorl_last_error()
        assert msg.startswith(name.encode() + b": ") and b"SOLORL_POLICY_MAX_WIDTH = 128" in msg, (name, msg)


def test_entry_points_reject_a_null_table(lib):
    P, B, W, G, S = _tables(79, 12)
    d = C.c_void_p(4096)
    calls = {"solorl_policy_act_w": lambda: lib.solorl_policy_act_w(None, d, None, None, 64, d, d, d, 0, None),
             "solorl_ppo_grad_stage1_w": lambda: lib.solorl_ppo_grad_stage1_w(None, C.byref(B), None, C.byref(W), None, 0, None),
             "solorl_ppo_grad_stage2_w": lambda: lib.solorl_ppo_grad_stage2_w(None, C.byref(W), None, 64, C.byref(G), 0, None),
             "solorl_ppo_clip_adam_w": lambda: lib.solorl_ppo_clip_adam_w(None, C.byref(G), C.byref(S), 0, None)}
    for name, call in calls.items():
        assert call() == -1, name
        assert lib.solorl_last_error() == name.encode() + b": null policy parameters"
    # ... and a table with a null parameter pointer, null arrays, rows that are no whole tiles
    P.mean_w = None
    for name, call in _calls(lib, P, B, W, G, S, False).items():
        assert call() == -1 and b"null policy parameter pointer" in lib.solorl_last_error(), name
    P, B, W, G, S = _tables(79, 12)
    assert lib.solorl_policy_act_w(C.byref(P), None, None, None, 64, d, d, d, 0, None) == -1
    assert lib.solorl_last_error() == b"solorl_policy_act_w: null array or n < 1"
    assert lib.solorl_ppo_grad_stage1_w(C.byref(P), None, None, C.byref(W), None, 0, None) == -1
    assert lib.solorl_ppo_grad_stage2_w(C.byref(P), None, None, 64, C.byref(G), 0, None) == -1
    assert lib.solorl_last_error() == b"solorl_ppo_grad_stage2_w: null argument or m < 1"
    assert lib.solorl_ppo_clip_adam_w(C.byref(P), None, C.byref(S), 0, None) == -1
    assert lib.solorl_last_error() == b"solorl_ppo_clip_adam_w: null argument"
    B.m = 48
    assert lib.solorl_ppo_grad_stage1_w(C.byref(P), C.byref(B), None, C.byref(W), None, 0, None) == -1 and b"multiple of 32" in lib.solorl_last_error()
    assert lib.solorl_ppo_grad_stage2_w(C.byref(P), C.byref(W), None, 96, C.byref(G), 0, None) == -1 and b"multiple of 64" in lib.solorl_last_error()
    # the 32-bit index bound and the alignment rule of rows whose width is a multiple of 4
    B.m = 1 << 25                                     # x 79 words >= 2^31
    assert lib.solorl_ppo_grad_stage1_w(C.byref(P), C.byref(B), None, C.byref(W), None, 0, None) == -1 and b"indexed with 32 bits" in lib.solorl_last_error()
    P4, B4, W4, G4, S4 = _tables(84, 12)
    assert lib.solorl_policy_act_w(C.byref(P4), C.c_void_p(4100), None, None, 64, d, d, d, 0, None) == -1 and b"16-byte aligned" in lib.solorl_last_error()
    if not torch.cuda.is_available():                 # 79 words are read word by word: accepted (never with a device: the arrays are dummies)
        assert lib.solorl_policy_act_w(C.byref(P), C.c_void_p(4100), None, None, 64, d, d, d, 0, None) == -2


def test_critic_arrays_go_with_a_critic_width_and_only_with_one(lib):
    P, B, W, G, S = _tables(79, 12)                   # symmetric: the critic's arrays are refused
    for name, call in _calls(lib, P, B, W, G, S, True).items():
        if name == "solorl_ppo_clip_adam_w":
            continue                                  # (takes no arrays of the critic's)
        assert call() == -1, name
        assert lib.solorl_last_error().startswith(name.encode() + b": ") and b"critic_obs_dim is 0" in lib.solorl_last_error(), name
    P, B, W, G, S = _tables(79, 12, critic_obs_dim=96)
    for name, call in _calls(lib, P, B, W, G, S, False).items():
        if name == "solorl_ppo_clip_adam_w":
            continue
        assert call() == -1, name
        assert lib.solorl_last_error().startswith(name.encode() + b": ") and b"critic's arrays are NULL" in lib.solorl_last_error(), name
    d = C.c_void_p(4096)                              # stage 1 takes two of them: both or neither
    assert lib.solorl_ppo_grad_stage1_w(C.byref(P), C.byref(B), d, C.byref(W), None, 0, None) == -1 and b"both or neither" in lib.solorl_last_error()


@pytest.mark.parametrize("obs,critic,act", [(79, 0, 12), (79, 96, 12), (128, 1, 8), (1, 128, 8), (76, 0, 12)])
def test_a_shape_inside_the_cap_reaches_the_device_lookup(lib, obs, critic, act):
    """without a GPU: -2, "no CPU fallback" -- every check of the shape and the arguments has passed by then.  (With one, the dummy
    arrays must not be launched on: nothing to see here.)"""
    if torch.cuda.is_available():
        return
    P, B, W, G, S = _tables(obs, act, 64, critic)
    for name, call in _calls(lib, P, B, W, G, S, critic != 0).items():
        assert call() == -2, (name, lib.solorl_last_error())
        assert b"no CPU fallback" in lib.solorl_last_error()


def _cpu_policy(O, OC, A):
    from solorl_amd.ppo import Policy
    from solorl_amd.vec_env import Box
    return Policy((O,), Box(-np.ones(A), np.ones(A)), None, {"hidden_size": 64}, **({} if OC is None else {"critic_obs_dim": OC}))


def test_the_family_chooser_and_the_switch(monkeypatch):
    from solorl_amd.ppo import fused, graphs
    from solorl_amd.ppo.fused import GENERIC, TEMPLATED, shape_kernel_family
    # the switch unset: the family built per shape, or none -- today's behaviour
    monkeypatch.delenv("SOLORL_POLICY_GENERIC", raising=False)
    assert graphs._generic_switch() == 0
    assert shape_kernel_family(76, None, 12) == TEMPLATED and shape_kernel_family(79, None, 12) is None
    assert shape_kernel_family(76, 96, 12) == TEMPLATED and shape_kernel_family(79, 96, 12) is None and shape_kernel_family(76, 76, 12) is None
    # 1: the generic family where the other builds nothing; 2: wherever it can run
    assert shape_kernel_family(76, None, 12, generic=1) == TEMPLATED and shape_kernel_family(79, None, 12, generic=1) == GENERIC
    assert shape_kernel_family(76, None, 12, generic=2) == GENERIC and shape_kernel_family(76, 96, 12, generic=2) == GENERIC
    assert shape_kernel_family(129, None, 12, generic=2) is None and shape_kernel_family(84, 129, 12, generic=1) is None
    assert shape_kernel_family(79, None, 16, generic=1) is None and shape_kernel_family(79, None, 12, h=32, generic=1) is None
    assert shape_kernel_family(79, 79, 12, generic=2) is None                  # (a critic width that equals obs is written None)
    monkeypatch.setenv("SOLORL_POLICY_GENERIC", "1")
    assert graphs._generic_switch() == 1
    # parameters the kernels cannot read -- CPU tensors -- have no family, whatever the switch says
    for shape in ((76, None, 12), (79, None, 12), (79, 96, 12)):
        pol = _cpu_policy(*shape)
        assert not fused.policy_kernels_generic_supported(pol) and not fused.policy_kernels_supported(pol)
        assert fused.policy_kernel_family(pol, 2) is None and graphs._policy_family(pol) is None
        assert fused._policy_shape(pol) == shape + (64,)


def test_train_script_flag_sets_the_switch(monkeypatch):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(root)
    import train_ppo
    assert train_ppo.get_ppo_args([]).generic_policy_kernels is False
    assert train_ppo.get_ppo_args(["--generic-policy-kernels"]).generic_policy_kernels is True
