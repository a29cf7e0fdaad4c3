"""Shared by tests/test_kin_static.py and tests/test_dyn_static.py: what the built code object says about a row-query kernel, the
members a struct of include/solorl.h declares, and the arguments every row query refuses."""
import ctypes as C
import os
import re

from solorl_amd import build, devcode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def residency(prefix):
    """``prefix``: kin or dyn -> (ENVS of csrc/solorl_<prefix>.hip, [(kernel name, its resources, static LDS bytes, workgroups per CU
    by registers, by LDS)] for the Solo8 and the Solo12 kernel).  Residency from BOTH limits, as the hardware counts them: LDS (160 KiB
    per CU) and registers (a SIMD holds floor(512 / allocated registers) wavefronts, registers allocated in blocks of 8, VGPRs and
    AGPRs together; four SIMDs per CU).  Neither the kernels nor sincos_call touch scratch or use FLAT accesses."""
    kernel = prefix + "_rows_kernel"
    res = {k: v for k, v in devcode.kernel_resources(build.LIB).items() if kernel in k}
    assert len(res) == 2, sorted(res)                       # Solo8 and Solo12
    src = open(os.path.join(ROOT, "solorl_amd", "csrc", "solorl_%s.hip" % prefix)).read()
    envs = int(re.search(r"constexpr int %s_ENVS = (\d+);" % prefix.upper(), src).group(1))
    waves = int(re.search(r"constexpr int %s_WAVES = (\d+);" % prefix.upper(), src).group(1))
    out = []
    for name, r in res.items():
        assert r["private_segment_fixed_size"] == 0, (name, r)          # no scratch: nothing spilled, nothing indexed by data
        lds = r["group_segment_fixed_size"]
        regs = r["vgpr_count"] + r.get("agpr_count", 0)
        waves_per_simd = min(8, 512 // (-(-regs // 8) * 8))
        out.append((name, r, lds, 4 * waves_per_simd // waves, (160 * 1024) // lds))
    stats = {k: v for k, v in devcode.function_stats(build.LIB).items() if kernel in k or "sincos_call" in k}
    assert len(stats) >= 3, sorted(stats)
    for name, s in stats.items():
        assert s["scratch"] == 0 and s["flat"] == 0, (name, s)
    return envs, out


def declared_members(struct, dims):
    """(header text, [(member, shape)] of ``typedef struct <struct>`` in include/solorl.h, all doubles; dims: macro -> value)"""
    hdr = open(os.path.join(ROOT, "include", "solorl.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    dims = {d: int(re.search(r"#define %s (\d+)" % d, hdr).group(1)) for d in dims}
    declared = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        assert stmt.startswith("double "), stmt
        for d in stmt[len("double "):].split(","):
            m = re.match(r"\s*(\w+)((?:\[\w+\])*)\s*$", d)
            declared.append((m.group(1), tuple(int(dims.get(x, x)) for x in re.findall(r"\[(\w+)\]", m.group(2)))))
    return hdr, dims, declared


def assert_refused(entry, cfg, bad_cfgs):
    """null cfg / states / out, n < 1 and every config of ``bad_cfgs``: -1 (SOLORL_ERR_INVALID), the message names the function"""
    from solorl_amd import _native
    lib, p = _native.lib(), C.c_void_p(4096)
    calls = [(None, p, p, 4), (C.byref(cfg), None, p, 4), (C.byref(cfg), p, None, 4), (C.byref(cfg), p, p, 0), (C.byref(cfg), p, p, -3)]
    for c, s, o, n in calls + [(C.byref(b), p, p, 4) for b in bad_cfgs]:
        assert getattr(lib, entry)(c, s, None, n, o, 0, None) == -1
        assert lib.solorl_last_error().startswith(entry.encode() + b":"), lib.solorl_last_error()
