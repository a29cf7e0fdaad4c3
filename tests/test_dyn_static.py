"""Static checks of solorl_dynamics (no GPU): the built kernels use no scratch, no AGPRs and no FLAT access, their static LDS is the
staged rows and nothing else, the workgroups per CU that registers and LDS allow are what DESIGN.md states (read from the code object's
metadata, as tests/test_kin_static.py does), the Python mirror of solorl_env_dyn agrees with the header, and the arguments the entry
point must refuse are refused before any HIP call."""
import ctypes as C
import os
import re

import pytest

from solorl_amd import _native, build, devcode
from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
from solorl_amd import dyn_tensors as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


def test_kernels_use_no_scratch_no_agprs_and_design_states_their_residency(lib):
    """Residency from BOTH limits, as the hardware counts them: LDS (160 KiB per CU) and registers (a SIMD holds floor(512 / allocated
    registers) wavefronts, registers allocated in blocks of 8; four SIMDs per CU)."""
    res = {k: v for k, v in devcode.kernel_resources(build.LIB).items() if "dyn_rows_kernel" in k}
    assert len(res) == 2, sorted(res)                       # Solo8 and Solo12
    src = open(os.path.join(ROOT, "solorl_amd", "csrc", "solorl_dyn.hip")).read()
    envs = int(re.search(r"constexpr int DYN_ENVS = (\d+);", src).group(1))
    waves = int(re.search(r"constexpr int DYN_WAVES = (\d+);", src).group(1))
    assert envs == D.ENVS_PER_WORKGROUP
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    stated = int(re.search(r"`dyn_rows_kernel`: (\d+) workgroups? resident per CU", design).group(1))
    assert stated >= 1
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (name, r)
        assert r.get("agpr_count", 0) == 0, (name, r)
        lds = r["group_segment_fixed_size"]
        assert lds == envs * (37 + D.ROW_WORDS) * 8 + envs * 4, (name, r)   # staged rows in and out plus the rows' live flags
        regs = r["vgpr_count"] + r.get("agpr_count", 0)
        waves_per_simd = min(8, 512 // (-(-regs // 8) * 8))
        by_regs, by_lds = 4 * waves_per_simd // waves, (160 * 1024) // lds
        assert min(by_regs, by_lds) == stated, (name, regs, lds, by_regs, by_lds, stated)
    stats = {k: v for k, v in devcode.function_stats(build.LIB).items() if "dyn_rows_kernel" in k or "sincos_call" in k}
    assert len(stats) >= 3, sorted(stats)
    for name, s in stats.items():
        assert s["scratch"] == 0 and s["flat"] == 0, (name, s)


def test_python_mirror_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "solorl.h")).read()
    body = re.search(r"typedef struct solorl_env_dyn \{(.*?)\} solorl_env_dyn;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    dims = {"SOLORL_DYN_NV": int(re.search(r"#define SOLORL_DYN_NV (\d+)", hdr).group(1))}
    declared = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        assert stmt.startswith("double "), stmt
        for d in stmt[len("double "):].split(","):
            m = re.match(r"\s*(\w+)((?:\[\w+\])*)\s*$", d)
            declared.append((m.group(1), tuple(int(dims.get(x, x)) for x in re.findall(r"\[(\w+)\]", m.group(2)))))
    assert declared == [(n, D.MEMBERS[n][1]) for n, _ in D.EnvDyn._fields_]
    assert [n for n, _ in declared] == ["mass_matrix", "bias", "gravity", "foot_jac", "foot_acc_bias", "foot_pos"]
    assert D.ROW_BYTES == 4800 and D.ROW_WORDS == 600 and D.NV == dims["SOLORL_DYN_NV"] == 18
    assert re.search(r"#define SOLORL_ABI_VERSION 5\b", hdr)             # no existing struct changed
    assert re.search(r"^ \*   solorl_dynamics ", hdr, re.M)              # the header's opening list names the entry point


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """null cfg / states / out, n < 1, a bad robot, a non-finite gravity, a non-finite or negative damping: SOLORL_ERR_INVALID, the
    message names the function -- on a machine without a GPU too, so the check precedes the first HIP call (which would answer
    SOLORL_ERR_NODEVICE there)"""
    cfg = default_config(ROBOT_SOLO12, TASK_WALK)
    p = C.c_void_p(4096)

    def with_(**kw):
        c = cfg.copy()
        for k, v in kw.items():
            setattr(c, k, v)
        return C.byref(c)

    calls = [(None, p, p, 4), (C.byref(cfg), None, p, 4), (C.byref(cfg), p, None, 4), (C.byref(cfg), p, p, 0), (C.byref(cfg), p, p, -3),
             (with_(robot=2), p, p, 4), (with_(robot=-1), p, p, 4), (with_(gravity=float("nan")), p, p, 4), (with_(gravity=float("inf")), p, p, 4),
             (with_(damping=float("nan")), p, p, 4), (with_(damping=float("inf")), p, p, 4), (with_(damping=-0.04), p, p, 4)]
    for c, s, o, n in calls:
        assert lib.solorl_dynamics(c, s, None, n, o, 0, None) == -1
        assert lib.solorl_last_error().startswith(b"solorl_dynamics:"), lib.solorl_last_error()
