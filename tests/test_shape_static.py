"""Static checks of solorl_shape_reward (no GPU): the built kernels use no scratch, no AGPRs and no FLAT access, their static LDS is
exactly the staged words SHAPE_ENVS implies, and the workgroups a CU holds by registers and by LDS are what DESIGN.md states; the
Python mirrors of solorl_shape_params and solorl_env_shape agree with the header, which still has ABI version 5; and the arguments
the entry point must refuse are refused before any HIP call."""
import ctypes as C
import math
import os
import re

import pytest

from solorl_amd import _native, build
from solorl_amd import shaping as S
from solorl_amd.config import default_config, ROBOT_SOLO8, ROBOT_SOLO12, TASK_WALK
from tests import rows_util as ru

# one env's LDS row (csrc/solorl_shape.hip): 54 staged state words, the 45-word memory row, 4 x 7 foot words, 16 terms
LDS_ROW_WORDS = 54 + S.ROW_WORDS + 28 + S.SHAPE_TERMS


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


def test_kernels_use_no_scratch_and_fit_a_cu_as_design_md_says(lib):
    envs, kernels = ru.residency("shape")        # (holds the kernels and sincos_call to no scratch and no FLAT access)
    assert envs == S.ENVS_PER_WORKGROUP
    design = open(os.path.join(ru.ROOT, "DESIGN.md")).read()
    stated = int(re.search(r"`shape_rows_kernel`: (\d+) workgroups per CU", design).group(1))
    for name, r, lds, by_regs, by_lds in kernels:
        assert r.get("agpr_count", 0) == 0, (name, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (name, r)
        assert lds == envs * LDS_ROW_WORDS * 8 + envs * 4, (name, lds)      # the rows and their live flags, nothing else
        assert min(by_regs, by_lds) == stated == 2, (name, r, lds, by_regs, by_lds)
    assert LDS_ROW_WORDS % 2 == 1                                             # lane = row accesses at one offset: no bank conflict


def test_python_mirrors_match_the_header():
    hdr = open(os.path.join(ru.ROOT, "include", "solorl.h")).read()
    assert re.search(r"#define SOLORL_ABI_VERSION 5\b", hdr)                 # no existing struct changed
    assert int(re.search(r"#define SOLORL_SHAPE_TERMS (\d+)", hdr).group(1)) == len(S.TERMS) == S.SHAPE_TERMS == 16
    assert C.sizeof(S.EnvShape) == 360 and S.ROW_WORDS == 45 and C.sizeof(S.ShapeParams) == 8 * (16 + 8)

    def members(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for stmt in body.split(";"):
            stmt = stmt.strip()
            if stmt:
                ctype, rest = stmt.split(None, 1)
                for d in rest.split(","):
                    m = re.match(r"\s*(\w+)(?:\[(\w+)\])?\s*$", d)
                    out.append((m.group(1), ctype, {None: 0, "SOLORL_SHAPE_TERMS": 16}.get(m.group(2), m.group(2))))
        return [(n, t, int(k)) for n, t, k in out]

    def mirror(cls):
        return [(n, "double" if (t._type_ if hasattr(t, "_length_") else t) is C.c_double else "int32_t", getattr(t, "_length_", 0)) for n, t in cls._fields_]
    assert members("solorl_shape_params") == mirror(S.ShapeParams)
    assert members("solorl_env_shape") == mirror(S.EnvShape)
    # the header's term table names the terms in TERMS' order
    table = re.findall(r"^ \*\s+(\d+)\s+(\w+)\s{2,}\S", hdr, re.M)
    assert [(int(k), n) for k, n in table if n in S.TERMS] == list(enumerate(S.TERMS))
    # the opening list names the entry point, and the binding knows it
    assert re.search(r"^ \*   solorl_shape_reward\s+<-", hdr, re.M) and "solorl_shape_reward" in _native.SYMBOLS
    mem = S.ShapeMem(3, "cpu")
    assert mem.data.shape == (3, 45) and mem.ep_sum.shape == (3, 16) and mem.prev_action.shape == (3, 12) and mem.air_time.shape == (3, 4)
    mem.valid[1] = 1; mem.prev_contact[2] = 5
    assert mem.data.view(__import__("torch").int32)[1, 89] == 1 and mem.data.view(__import__("torch").int32)[2, 88] == 5


def test_unknown_names_are_refused_by_name():
    with pytest.raises(ValueError, match="foot_slop"):
        S.make_params({"foot_slop": 1.0})
    with pytest.raises(ValueError, match="sigma"):
        S.make_params({"foot_slip": 1.0}, sigma=2.0)
    with pytest.raises(ValueError, match="weights"):
        S.params_from_dict({"foot_slip": 1.0})
    p = S.params_from_dict({"weights": {"foot_slip": -0.5}, "cmd_lin_vel": [0.3, 0.1]})
    assert p.weight[S.TERMS.index("foot_slip")] == -0.5 and sum(1 for w in p.weight if w) == 1 and tuple(p.cmd_lin_vel) == (0.3, 0.1)


def test_example_file_and_launcher_flag(tmp_path):
    """configs/shaping_walk12.yaml names known terms and parameters only; train_ppo.py parses --reward-shaping and refuses a file with an
    unknown term by its name, before anything is built"""
    import sys
    import yaml
    sys.path.insert(0, ru.ROOT)
    import train_ppo
    path = os.path.join(ru.ROOT, "configs", "shaping_walk12.yaml")
    p = S.params_from_dict(yaml.safe_load(open(path)))
    assert sum(1 for w in p.weight if w) >= 8 and p.tracking_sigma > 0
    assert "UNTUNED" in open(path).read()
    assert train_ppo.get_ppo_args(["--reward-shaping", path]).reward_shaping == path and train_ppo.get_ppo_args([]).reward_shaping is None
    bad = tmp_path / "bad.yaml"
    bad.write_text("weights:\n  foot_slop: -1.0\n")
    with pytest.raises(SystemExit, match="foot_slop"):
        train_ppo.main(["--config-file", os.path.join(ru.ROOT, "configs", "basic12.yaml"), "--reward-shaping", str(bad)])


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """null cfg / p / states / actions / mem, n < 1, a bad robot, a non-finite weight or parameter, tracking_sigma <= 0, sim_dt <= 0,
    frame_skip < 1: SOLORL_ERR_INVALID, the message starts with the function's name -- on a machine without a GPU too, so the check
    precedes the first HIP call (which would answer SOLORL_ERR_NODEVICE there)"""
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    good = S.make_params({"foot_slip": -1.0})
    x = C.c_void_p(4096)

    def call(cfg=cfg, p=good, states=x, actions=x, mem=x, n=4):
        rc = lib.solorl_shape_reward(None if cfg is None else C.byref(cfg), None if p is None else C.byref(p), states, None, n, actions, None, mem,
                                     None, None, None, 0, None)
        assert rc == -1, rc
        assert lib.solorl_last_error().startswith(b"solorl_shape_reward:"), lib.solorl_last_error()

    for kw in (dict(cfg=None), dict(p=None), dict(states=None), dict(actions=None), dict(mem=None), dict(n=0), dict(n=-3)):
        call(**kw)
    for robot in (2, -1):
        c = cfg.copy(); c.robot = robot
        call(cfg=c)
    for dt in (0.0, -1.0 / 240, float("nan"), float("inf")):
        c = cfg.copy(); c.sim_dt = dt
        call(cfg=c)
    for fs in (0, -4):
        c = cfg.copy(); c.frame_skip = fs
        call(cfg=c)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(C.sizeof(S.ShapeParams) // 8):          # every weight and every parameter
            p = S.make_params({"foot_slip": -1.0})
            (C.c_double * (C.sizeof(S.ShapeParams) // 8)).from_buffer(p)[k] = bad
            call(p=p)
    for sigma in (0.0, -0.25):
        call(p=S.make_params({"foot_slip": -1.0}, tracking_sigma=sigma))
    assert math.isfinite(good.tracking_sigma) and good.tracking_sigma > 0
