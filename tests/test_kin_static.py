"""Static checks of solorl_kinematics (no GPU): the built kernels use no scratch and two workgroups of them fit a CU by registers and by LDS (read from
the code object's metadata, as tests/test_abi.py does for the step kernels), the Python mirror of solorl_env_kin agrees with the
header, and the arguments the entry point must refuse are refused before any HIP call."""
import ctypes as C
import os
import re

import pytest

from solorl_amd import _native, build, devcode
from solorl_amd.config import default_config, ROBOT_SOLO8, ROBOT_SOLO12, TASK_WALK
from solorl_amd import kinematics as K
from solorl_amd.state import ROW_BYTES as STATE_ROW_BYTES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


def test_kernels_use_no_scratch_and_two_workgroups_fit_a_cu(lib):
    """Residency from BOTH limits, as the hardware counts them: LDS (160 KiB per CU) and registers (a SIMD holds floor(512 / allocated
    registers) wavefronts, registers allocated in blocks of 8, VGPRs and AGPRs together; four SIMDs per CU)."""
    res = {k: v for k, v in devcode.kernel_resources(build.LIB).items() if "kin_rows_kernel" in k}
    assert len(res) == 2, sorted(res)                       # Solo8 and Solo12
    src = open(os.path.join(ROOT, "solorl_amd", "csrc", "solorl_kin.hip")).read()
    envs = int(re.search(r"constexpr int KIN_ENVS = (\d+);", src).group(1))
    waves = int(re.search(r"constexpr int KIN_WAVES = (\d+);", src).group(1))
    assert envs == K.ENVS_PER_WORKGROUP
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0, (name, r)          # no scratch: nothing spilled, nothing indexed by data
        lds = r["group_segment_fixed_size"]
        assert lds == envs * (74 + K.ROW_WORDS) * 8 + envs * 4, (name, r)   # staged rows in and out plus the rows' live flags
        regs = r["vgpr_count"] + r.get("agpr_count", 0)
        waves_per_simd = min(8, 512 // (-(-regs // 8) * 8))
        by_regs, by_lds = 4 * waves_per_simd // waves, (160 * 1024) // lds
        assert min(by_regs, by_lds) == 2, (name, regs, lds, by_regs, by_lds)    # what DESIGN.md and the kernel's comment say
    stats = {k: v for k, v in devcode.function_stats(build.LIB).items() if "kin_rows_kernel" in k or "sincos_call" in k}
    assert len(stats) >= 3, sorted(stats)
    for name, s in stats.items():
        assert s["scratch"] == 0 and s["flat"] == 0, (name, s)


def test_python_mirror_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "solorl.h")).read()
    body = re.search(r"typedef struct solorl_env_kin \{(.*?)\} solorl_env_kin;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    dims = {"SOLORL_KIN_MAX_LINKS": int(re.search(r"#define SOLORL_KIN_MAX_LINKS (\d+)", hdr).group(1)),
            "SOLORL_STATE_MAX_PRIMS": int(re.search(r"#define SOLORL_STATE_MAX_PRIMS (\d+)", hdr).group(1))}
    declared = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        assert stmt.startswith("double "), stmt
        for d in stmt[len("double "):].split(","):
            m = re.match(r"\s*(\w+)((?:\[\w+\])*)\s*$", d)
            declared.append((m.group(1), tuple(int(dims.get(x, x)) for x in re.findall(r"\[(\w+)\]", m.group(2)))))
    assert declared == [(n, K.MEMBERS[n][1]) for n, _ in K.EnvKin._fields_]
    assert K.ROW_BYTES == 3640 and STATE_ROW_BYTES == 2040 and K.KIN_MAX_LINKS == dims["SOLORL_KIN_MAX_LINKS"]
    assert len(K.LINK_NAMES[ROBOT_SOLO8]) == 13 and len(K.LINK_NAMES[ROBOT_SOLO12]) == 17
    assert K.LINK_NAMES[ROBOT_SOLO12][0] == "base_link" and K.LINK_NAMES[ROBOT_SOLO12][4] == "FL_FOOT"
    assert re.search(r"#define SOLORL_ABI_VERSION 5\b", hdr)             # no existing struct changed


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """null cfg / states / out, n < 1, a bad robot, sim_dt <= 0: SOLORL_ERR_INVALID, the message names the function -- on a machine
    without a GPU too, so the check precedes the first HIP call (which would answer SOLORL_ERR_NODEVICE there)"""
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    p = C.c_void_p(4096)
    bad_robot = cfg.copy(); bad_robot.robot = 2
    bad_dt = cfg.copy(); bad_dt.sim_dt = 0.0
    neg_dt = cfg.copy(); neg_dt.sim_dt = -1.0 / 240
    nan_dt = cfg.copy(); nan_dt.sim_dt = float("nan")
    calls = [(None, p, p, 4), (C.byref(cfg), None, p, 4), (C.byref(cfg), p, None, 4), (C.byref(cfg), p, p, 0), (C.byref(cfg), p, p, -3),
             (C.byref(bad_robot), p, p, 4), (C.byref(bad_dt), p, p, 4), (C.byref(neg_dt), p, p, 4), (C.byref(nan_dt), p, p, 4)]
    for c, s, o, n in calls:
        assert lib.solorl_kinematics(c, s, None, n, o, 0, None) == -1
        assert lib.solorl_last_error().startswith(b"solorl_kinematics:"), lib.solorl_last_error()
