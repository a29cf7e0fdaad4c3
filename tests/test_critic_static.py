"""Static checks of solorl_critic_obs (no GPU): the header declares the call and its table and still has ABI version 5, the Python
mirror of solorl_critic_params agrees with it, the built kernels use no scratch, no AGPRs and no FLAT access and the workgroups a CU
holds by registers and by LDS are what DESIGN.md states; the arguments the entry point must refuse are refused before any HIP call; the
scale names, the example file and the launcher flag; the stage's entry in the env's stage table."""
import ctypes as C
import os
import re
import types

import pytest

from solorl_amd import _native, build
from solorl_amd import critic_obs as K
from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
from tests import rows_util as ru

LDS_ROW_WORDS = 55 + 28       # one env's LDS row (csrc/solorl_critic.hip): 55 staged state words, 4 x 7 foot words


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


def test_header_declares_the_call_and_keeps_abi_5():
    hdr = open(os.path.join(ru.ROOT, "include", "solorl.h")).read()
    assert re.search(r"#define SOLORL_ABI_VERSION 5\b", hdr)                 # no existing struct changed
    assert int(re.search(r"#define SOLORL_CRITIC_PRIV (\d+)", hdr).group(1)) == _native.CRITIC_PRIV == 20
    assert re.search(r"^int solorl_critic_obs\(const solorl_config\* cfg, const solorl_critic_params\* p,", hdr, re.M)
    assert "solorl_critic_obs" in _native.SYMBOLS
    body = re.search(r"typedef struct solorl_critic_params \{(.*?)\} solorl_critic_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [s.strip() for s in body.split(";") if s.strip()] == ["double scale[SOLORL_CRITIC_PRIV]", "int32_t obs_dim", "int32_t reserved"]
    assert [(n, getattr(t, "_length_", 0)) for n, t in _native.CriticParams._fields_] == [("scale", 20), ("obs_dim", 0), ("reserved", 0)]
    assert C.sizeof(_native.CriticParams) == 8 * 20 + 8 and _native.CriticParams.obs_dim.offset == 160
    # the structs the call reads rows of are the ones the earlier stages own, unchanged
    assert C.sizeof(_native.EnvActuator) == 256 and C.sizeof(_native.EnvCommand) == 32 and C.sizeof(_native.PolicyParams) == 16 + 13 * 8
    # the table's rows, in the order of the groups of critic_obs.GROUPS
    table = re.search(r"k\s+raw_k\n(.*?)Nothing is done about non-finite", hdr, re.S).group(1)
    firsts = [int(m) for m in re.findall(r"^ \*\s{4}(\d+)(?:\.\.\d+)?\s{2,}\S", table, re.M)]
    assert firsts == [first for first, _ in K.GROUPS.values()]


def test_kernels_use_no_scratch_and_fit_a_cu_as_design_md_says(lib):
    envs, kernels = ru.residency("critic")       # (holds the kernels and sincos_call to no scratch and no FLAT access)
    assert envs == K.ENVS_PER_WORKGROUP == 64
    design = open(os.path.join(ru.ROOT, "DESIGN.md")).read()
    stated = int(re.search(r"`critic_rows_kernel`: (\d+) workgroups per CU", design).group(1))
    for name, r, lds, by_regs, by_lds in kernels:
        assert r.get("agpr_count", 0) == 0, (name, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert lds == envs * (LDS_ROW_WORDS * 8 + 4 + 20 * 4), (name, lds)      # the rows, their live flags and the twenty words as floats
        assert min(by_regs, by_lds) == stated == 3, (name, r, lds, by_regs, by_lds)
    assert LDS_ROW_WORDS % 2 == 1                                                # lane = row accesses at one offset: no bank conflict


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """null cfg / p / states / obs_in / critic_out, n < 1, a bad robot, obs_dim < 1 or > 210, a non-finite scale: SOLORL_ERR_INVALID,
    the message starts with the function's name -- on a machine without a GPU too, so the check precedes the first HIP call"""
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    good = K.make_params(cfg, 76)
    x = C.c_void_p(4096)

    def call(cfg=cfg, p=good, states=x, obs=x, out=x, n=4):
        rc = lib.solorl_critic_obs(None if cfg is None else C.byref(cfg), None if p is None else C.byref(p), states, None, n, obs, None, None, None,
                                   out, 0, None)
        assert rc == -1, rc
        assert lib.solorl_last_error().startswith(b"solorl_critic_obs:"), lib.solorl_last_error()

    for kw in (dict(cfg=None), dict(p=None), dict(states=None), dict(obs=None), dict(out=None), dict(n=0), dict(n=-3)):
        call(**kw)
    for robot in (2, -1):
        c = cfg.copy(); c.robot = robot
        call(cfg=c)
    for E in (0, -1, 211):
        p = K.make_params(cfg, 76); p.obs_dim = E
        call(p=p)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(20):
            p = K.make_params(cfg, 76); p.scale[k] = bad
            call(p=p)


def test_scales_defaults_and_unknown_names():
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    p = K.make_params(cfg, 76)
    assert p.obs_dim == 76 and p.scale[15] == 1.0 / cfg.episode_length and all(s != 0 for s in p.scale)
    p = K.make_params(cfg, 38, foot_force=[1, 2, 3, 4], command=0.5, kick=0.0)
    assert list(p.scale[0:4]) == [1, 2, 3, 4] and list(p.scale[12:15]) == [0.5] * 3 and p.scale[19] == 0.0
    with pytest.raises(ValueError, match="foot_farce"):
        K.make_params(cfg, 76, foot_farce=1.0)
    with pytest.raises(ValueError, match="foot_height"):
        K.make_params(cfg, 76, foot_height=[1.0, 2.0])
    with pytest.raises(ValueError, match="gain"):
        K.make_params(cfg, 76, gain=float("nan"))
    with pytest.raises(ValueError, match="1..210"):
        K.make_params(cfg, 211)
    with pytest.raises(ValueError, match="'scales'"):
        K.scales_from_dict({"scales": {}})


def test_example_file():
    import yaml
    path = os.path.join(ru.ROOT, "configs", "critic_walk12.yaml")
    d = yaml.safe_load(open(path))
    K.make_params(default_config(ROBOT_SOLO12, TASK_WALK), 76, **K.scales_from_dict(d))
    assert "UNTUNED" in open(path).read()


def test_the_stage_bars_the_policy_tail_and_k_step_launches():
    """on what the guards read of an env (tests/test_args_cpu.py builds such envs without the attribute: is_set must not need it)"""
    from solorl_amd.vec_env import SoloVecEnv, _STAGES
    entry = [s for s in _STAGES if s[0] == "critic_obs"]
    assert len(entry) == 1 and _STAGES[-1] is entry[0]
    base = dict(_norm_obs=False, last_kick=None, _shape_params=None, _noise_scale=None, _act=None, _cmd=None, _term=None, _rr=None, obs_dim=76,
                act_dim=12, get_property=lambda name: 1.0 if name == "step_n_one_launch" else 0.0)
    P = types.SimpleNamespace(obs_dim=76, act_dim=12, hidden=64)
    e = types.SimpleNamespace(**base)
    e.step_act_supported = lambda params: SoloVecEnv.step_act_supported(e, params)
    e._refuse = lambda *a, **kw: SoloVecEnv._refuse(e, *a, **kw)
    assert not entry[0][1](e) and SoloVecEnv.step_act_supported(e, P) and SoloVecEnv.rollout_supported(e, P)
    e._critic = object()
    assert entry[0][1](e) and not SoloVecEnv.step_act_supported(e, P) and not SoloVecEnv.rollout_supported(e, P)
    for name in ("step_act_inplace", "rollout_inplace"):
        with pytest.raises(_native.SoloRLError, match=r"%s with critic_obs(.|\n)*value from the actor's row" % name):
            SoloVecEnv._refuse(e, name, tail=True)
    with pytest.raises(_native.SoloRLError, match=r"step_n with critic_obs(.|\n)*rollout_supported\(\) is False"):
        SoloVecEnv._refuse(e, "step_n", k_step=True)
    with pytest.raises(_native.SoloRLError, match="step_n"):
        SoloVecEnv._no_critic_obs(e, "step_n")


def test_policy_params_slot_and_the_old_entry_points_refusal(lib):
    """reserved0's slot of solorl_policy_params is critic_obs_dim (same size, same layout); the entry points of the symmetric policy
    refuse critic_obs_dim = 96 and the new ones a shape that is not built -- before the device lookup, so without a GPU too -- and
    every shape refusal keeps the list of the symmetric shapes"""
    hdr = open(os.path.join(ru.ROOT, "include", "solorl.h")).read()
    body = re.search(r"typedef struct solorl_policy_params \{(.*?)\} solorl_policy_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ints = [w.strip() for stmt in body.split(";") if stmt.strip().startswith("int ") for w in stmt.strip()[4:].split(",")]
    assert ints == ["obs_dim", "act_dim", "hidden", "critic_obs_dim"] and "reserved0" not in body
    P = _native.PolicyParams
    assert [n for n, _ in P._fields_[:4]] == ints and P.critic_obs_dim.offset == 12 and P.critic_w0.offset == 16 and C.sizeof(P) == 16 + 13 * 8
    for name in ("solorl_policy_act_critic", "solorl_ppo_grad_stage1_critic", "solorl_ppo_grad_stage2_critic", "solorl_ppo_grad_count2",
                 "solorl_ppo_scratch_count2"):
        assert name in _native.SYMBOLS and re.search(r"^int %s\(" % name, hdr, re.M), name
    p = P()
    p.obs_dim, p.act_dim, p.hidden, p.critic_obs_dim = 76, 12, 64, 96
    for k, _t in P._fields_[4:]:
        setattr(p, k, 4096)                           # non-null, 16-byte aligned (never dereferenced on the host)
    x = C.c_void_p(4096)
    B, W, G, S = _native.PpoBatch(), _native.PpoStage1(), _native.PpoGrads(), _native.AdamState()
    for st in (B, W, G, S):
        for k, t in st._fields_:
            if t is C.c_void_p:
                setattr(st, k, 4096)
    B.m = 64
    old = {"solorl_policy_act": lambda: lib.solorl_policy_act(C.byref(p), x, None, 64, x, x, x, 0, None),
           "solorl_ppo_grad_stage1": lambda: lib.solorl_ppo_grad_stage1(C.byref(p), C.byref(B), C.byref(W), 0, None),
           "solorl_ppo_grad_stage2": lambda: lib.solorl_ppo_grad_stage2(C.byref(p), C.byref(W), 64, C.byref(G), 0, None)}
    for name, call in old.items():
        assert call() == -1, name
        msg = lib.solorl_last_error()
        assert b"critic_obs_dim must be 0" in msg and b"38, 42, 76 or 84 x 12; 30, 34, 60 or 68 x 8" in msg, (name, msg)
    new = {"solorl_policy_act_critic": lambda: lib.solorl_policy_act_critic(C.byref(p), x, x, None, 64, x, x, x, 0, None),
           "solorl_ppo_grad_stage1_critic": lambda: lib.solorl_ppo_grad_stage1_critic(C.byref(p), C.byref(B), x, C.byref(W), x, 0, None),
           "solorl_ppo_grad_stage2_critic": lambda: lib.solorl_ppo_grad_stage2_critic(C.byref(p), C.byref(W), x, 64, C.byref(G), 0, None),
           "solorl_ppo_clip_adam": lambda: lib.solorl_ppo_clip_adam(C.byref(p), C.byref(G), C.byref(S), 0, None)}
    for bad in (100, 0):                              # a critic width that is not built; a symmetric policy at the _critic entry points
        p.critic_obs_dim = bad
        for name, call in new.items():
            if bad == 0 and name == "solorl_ppo_clip_adam":
                continue                              # (serves both forms)
            assert call() == -1, (name, bad)
            assert b"38, 42, 76 or 84 x 12; 30, 34, 60 or 68 x 8" in lib.solorl_last_error(), (name, bad, lib.solorl_last_error())
    assert lib.solorl_ppo_grad_count2(76, 96, 12) == 64 * 97 + 64 * 77 + 2 * 64 * 65 + 65 + 12 * 65
    assert lib.solorl_ppo_grad_count2(76, 76, 12) == lib.solorl_ppo_grad_count(76, 12)
    assert lib.solorl_ppo_scratch_count2(76, 76, 12, 32768) == lib.solorl_ppo_scratch_count(76, 12, 32768)
    assert lib.solorl_ppo_scratch_count2(76, 96, 12, 32768) > lib.solorl_ppo_scratch_count(76, 12, 32768) and lib.solorl_ppo_scratch_count2(76, 96, 12, 0) == 0
