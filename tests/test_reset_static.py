"""Static checks of solorl_randomize_reset and solorl_restart_history (no GPU): the header declares both calls and the struct and still
has ABI version 5, the library exports them and _native binds them, the ctypes mirror of solorl_reset_randomization has the C struct's
size and offsets, every argument the calls must refuse is refused before any HIP call, make_reset_randomization builds the struct from
readable keys and refuses unknown ones by name, build.py lists the new file, the kernel's resources are what DESIGN.md states, the
launchers parse the new flag, the example file loads and make_vec_envs leaves the feature off by default."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys

import pytest

from solorl_amd import _native, build, reset_random
from solorl_amd.config import ROBOT_SOLO8, ROBOT_SOLO12, TASK_WALK, default_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "solorl.h")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


def test_header_declares_the_calls_and_keeps_the_abi_version():
    hdr = open(HDR).read()
    assert re.search(r"#define SOLORL_ABI_VERSION 5\b", hdr)
    assert re.search(r"typedef struct solorl_reset_randomization \{.*?\} solorl_reset_randomization;", hdr, re.S)
    assert re.search(r"^int solorl_randomize_reset\(const solorl_config\* cfg, const solorl_reset_randomization\* p,", hdr, re.M)
    assert re.search(r"^int solorl_restart_history\(solorl_env\* env, const uint8_t\* mask", hdr, re.M)
    assert re.search(r"^ \*   solorl_randomize_reset / solorl_restart_history :", hdr, re.M)            # the opening list
    for piece in ("(gid_lo, gid_hi, 16 k + b, 8)", "u = (word >> 8) * 2^-24", "d = (2 u - 1) * a", "fmin(fmax(q[j] + d, -joint_limit), +joint_limit)",
                  "quat <- Rz(psi) * quat * Rx(phi) * Ry(theta)", "pos.z <- pos.z + (clearance - zmin)", "k < 2^28", "masked (mask byte 0)",
                  "-0.0 survives", "bits 0..23 of contact_mask <- 0", "feet words of the next observation therefore read 0",
                  "or calls solorl_restart_history afterwards"):
        assert piece in hdr, piece


def test_library_exports_and_binding(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name, nargs in (("solorl_randomize_reset", 8), ("solorl_restart_history", 4)):
        assert name in exported and name in _native.SYMBOLS
        assert getattr(lib, name).restype is C.c_int and len(getattr(lib, name).argtypes) == nargs
    assert lib.solorl_abi_version() == 5                     # no existing struct changed


def test_ctypes_struct_equals_the_c_struct(tmp_path):
    """sizeof and every offset, from a program the host compiler builds against the header"""
    names = [n for n, _ in _native.ResetRandomization._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "solorl.h"\nint main(void) {\n  printf("%zu", sizeof(solorl_reset_randomization));\n'
                   + "".join('  printf(" %%zu", offsetof(solorl_reset_randomization, %s));\n' % n for n in names) + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = _native.ResetRandomization
    assert got == [C.sizeof(T)] + [getattr(T, n).offset for n in names]
    assert C.sizeof(T) == 16 + 8 * (12 + 12 + 3 + 3 + 4) + 8 == 296


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """Every refused argument returns SOLORL_ERR_INVALID with the function's name in front -- on a machine without a GPU too, so the
    check precedes the first HIP call (which would answer SOLORL_ERR_NODEVICE there)"""
    x = C.c_void_p(4096)
    nan, inf = float("nan"), float("inf")

    def call(robot=ROBOT_SOLO12, cfg=True, p=True, rows=x, count=x, n=4, device=0, cfg_robot=None, joint_limit=None, **fields):
        c = default_config(robot, TASK_WALK)
        if cfg_robot is not None:
            c.robot = cfg_robot
        if joint_limit is not None:
            c.joint_limit = joint_limit
        P = reset_random.make_reset_randomization(c if cfg_robot is None else default_config(robot, TASK_WALK), 3, 0, joint_pos=0.2, joint_vel=1.0,
                                                  lin_vel=0.3, ang_vel=0.3, yaw=3.14, roll=0.1, pitch=0.1, clearance=0.01)
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(P, v[0])[v[1]] = v[2]
            else:
                setattr(P, k, v)
        return lib.solorl_randomize_reset(C.byref(c) if cfg else None, C.byref(P) if p else None, rows, None, count, n, device, None)

    def refused(**kw):
        assert call(**kw) == -1, kw
        assert lib.solorl_last_error().startswith(b"solorl_randomize_reset:"), lib.solorl_last_error()

    cases = [dict(cfg=False), dict(p=False), dict(rows=None), dict(count=None), dict(n=0), dict(n=-5), dict(cfg_robot=2), dict(cfg_robot=-1),
             dict(yaw=-0.1), dict(yaw=nan), dict(yaw=inf), dict(yaw=3.15), dict(yaw=float.fromhex("0x1.921fb54442d19p+1")), dict(roll=-1.0), dict(roll=nan),
             dict(roll=3.2), dict(pitch=-1e-9), dict(pitch=inf), dict(pitch=4.0), dict(clearance=-0.01), dict(clearance=nan), dict(clearance=inf),
             dict(joint_limit=-1.0), dict(joint_limit=nan)]
    for j in (0, 7, 11):
        cases += [dict(a=("joint_pos", j, -0.1)), dict(a=("joint_pos", j, nan)), dict(a=("joint_vel", j, inf)), dict(a=("joint_vel", j, -2.0))]
    for k in (0, 2):
        cases += [dict(a=("lin_vel", k, -0.1)), dict(a=("lin_vel", k, nan)), dict(a=("ang_vel", k, inf)), dict(a=("ang_vel", k, -2.0))]
    for kw in cases:
        refused(**kw)
    # what is allowed passes the checks: what answers is the device check (a device id no machine has), before any launch
    for kw in (dict(), dict(robot=ROBOT_SOLO8), dict(yaw=math.pi, roll=math.pi, pitch=math.pi), dict(yaw=0.0, roll=0.0, pitch=0.0, clearance=0.0),
               dict(place_on_ground=0), dict(n=1), dict(joint_limit=0.0), dict(seed=2 ** 64 - 1, env_id_offset=-5)):
        assert call(device=2 ** 20, **kw) == -2, (kw, lib.solorl_last_error())
    # the history restart: null handle and null mask name the function
    assert lib.solorl_restart_history(None, x, None, None) == -1 and lib.solorl_last_error().startswith(b"solorl_restart_history:")


def test_make_reset_randomization_reads_the_keys_and_refuses_unknown_ones_by_name():
    c12, c8 = default_config(ROBOT_SOLO12, TASK_WALK), default_config(ROBOT_SOLO8, TASK_WALK)
    p = reset_random.make_reset_randomization(c12, (7 << 32) | 5, 130, joint_pos=0.2, joint_vel=[0.1 * j for j in range(12)], lin_vel=[0.3, 0.2, 0.1],
                                              ang_vel=0.4, yaw=3.14, roll=0.1, pitch=0.2, clearance=0.02)
    assert (p.seed, p.env_id_offset, p.place_on_ground) == ((7 << 32) | 5, 130, 1)
    assert list(p.joint_pos) == [0.2] * 12 and list(p.joint_vel) == [0.1 * j for j in range(12)]
    assert list(p.lin_vel) == [0.3, 0.2, 0.1] and list(p.ang_vel) == [0.4] * 3
    assert (p.yaw, p.roll, p.pitch, p.clearance) == (3.14, 0.1, 0.2, 0.02)
    q = reset_random.make_reset_randomization(c8, 1, 0, joint_pos=0.2, joint_vel=[1.0] * 8, place_on_ground=False)
    assert list(q.joint_pos) == [0.2] * 8 + [0.0] * 4 and list(q.joint_vel) == [1.0] * 8 + [0.0] * 4 and q.place_on_ground == 0
    z = reset_random.make_reset_randomization(c12, 1, 0)                      # nothing named: every member an exact no-op but the placing
    assert not any(list(z.joint_pos) + list(z.joint_vel) + list(z.lin_vel) + list(z.ang_vel) + [z.yaw, z.roll, z.pitch, z.clearance]) and z.place_on_ground == 1
    with pytest.raises(ValueError, match="heading"):
        reset_random.make_reset_randomization(c12, 1, 0, heading=1.0)
    with pytest.raises(ValueError, match="jointpos"):
        reset_random.ranges_from_dict({"jointpos": 0.1})
    for bad in (dict(joint_pos=-0.1), dict(joint_pos=[0.1] * 8), dict(joint_vel=float("nan")), dict(lin_vel=[0.1, 0.2]), dict(ang_vel=float("inf")),
                dict(yaw=3.2), dict(roll=-0.1), dict(pitch=float("nan")), dict(clearance=-0.01), dict(clearance=float("inf"))):
        with pytest.raises(ValueError):
            reset_random.make_reset_randomization(c12, 1, 0, **bad)
    with pytest.raises(ValueError):
        reset_random.make_reset_randomization(c8, 1, 0, joint_pos=[0.1] * 12)       # a Solo8 has eight joints


def test_build_lists_the_new_unit():
    assert "solorl_reset.hip" in build.UNITS and build.UNIT_SUBDIR["solorl_reset.hip"] == "reset"
    deps = {os.path.basename(d) for d in build.UNITS["solorl_reset.hip"]}
    assert {"solorl_reset.hip", "reset_random.hpp", "row_batch.hpp", "kinematics.hpp", "perturb.hpp", "solorl.h"} <= deps
    assert all(os.path.exists(d) for d in build.UNITS["solorl_reset.hip"])
    assert "restart_history_kernel" in open(build.UNITS["solorl_hip.hip"][0]).read()


def test_kernel_resources(lib):
    """The code-object metadata of both instantiations: the staged rows' static LDS, no scratch, no AGPRs, no vector spills, and few
    enough registers for eight wavefronts per SIMD -- LDS decides the residency, seven workgroups per CU"""
    from solorl_amd import devcode
    res = {k: v for k, v in devcode.kernel_resources(build.LIB).items() if "reset_rows_kernel" in k}
    assert len(res) == 2, sorted(res)
    for k, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 64 * ((37 + 4) * 8 + 4) == 21248, (k, r)
        assert r.get("agpr_count", 0) == 0 and r.get("vgpr_spill_count", 0) == 0, (k, r)
        assert r["vgpr_count"] <= 64, (k, r)
        assert (160 * 1024) // r["group_segment_fixed_size"] == 7 >= 2
    assert reset_random.ENVS_PER_WORKGROUP == 64
    hist = {k: v for k, v in devcode.kernel_resources(build.LIB).items() if "restart_history_kernel" in k}
    assert len(hist) == 4, sorted(hist)                      # fp32 / fp64 x Solo8 / Solo12
    for k, r in hist.items():
        assert r["private_segment_fixed_size"] == 0 and r.get("vgpr_spill_count", 0) == 0, (k, r)


def test_launchers_parse_the_new_flag():
    sys.path.insert(0, ROOT)
    import train_ppo
    assert train_ppo.get_ppo_args([]).reset_randomization is None               # default: off
    path = os.path.join(ROOT, "configs", "reset_walk12.yaml")
    assert train_ppo.get_ppo_args(["--reset-randomization", path]).reset_randomization == path
    out = subprocess.run([sys.executable, os.path.join(ROOT, "eval_ppo.py"), "--help"], capture_output=True, text=True, check=True).stdout
    assert "--reset-randomization" in out


def test_example_file_and_defaults(tmp_path):
    sys.path.insert(0, ROOT)
    import train_ppo
    from solorl_amd.config import config_from_dict, load_yaml
    from solorl_amd.vec_env import SoloVecEnv, make_vec_envs
    path = os.path.join(ROOT, "configs", "reset_walk12.yaml")
    assert "UNTUNED" in open(path).read()
    config = load_yaml(os.path.join(ROOT, "configs", "basic12.yaml"))
    d = train_ppo.load_reset_randomization(path, config)
    p = reset_random.make_reset_randomization(config_from_dict(config), 1, 0, **d)
    assert list(p.joint_pos) == [0.2] * 12 and list(p.joint_vel) == [1.0] * 12 and list(p.lin_vel) == [0.3] * 3 and list(p.ang_vel) == [0.3] * 3
    assert (p.yaw, p.roll, p.pitch, p.clearance, p.place_on_ground) == (3.14, 0.1, 0.1, 0.0, 1)
    bad = tmp_path / "bad.yaml"
    bad.write_text("joint_pos: 0.1\nheading: 3.0\n")
    with pytest.raises(SystemExit, match="heading"):
        train_ppo.main(["--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--reset-randomization", str(bad)])
    assert inspect.signature(make_vec_envs).parameters["reset_randomization"].default is None
    for name in ("set_reset_randomization", "_no_reset_randomization", "_randomize"):
        assert name in dir(SoloVecEnv)
