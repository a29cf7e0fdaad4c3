"""Static checks of solorl_terminate (no GPU): the header declares the call and the struct and still has ABI version 5, the library
exports the call and _native binds it, the ctypes mirror of solorl_termination has the C struct's size and offsets, every argument the
call must refuse is refused before any HIP call, make_termination builds the struct from readable keys and refuses unknown ones by
name, the kernel's resources are what DESIGN.md states, the launchers parse the new flag, the example file loads and make_vec_envs
leaves the termination off by default."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys

import pytest

from solorl_amd import _native, build, termination
from solorl_amd.config import ROBOT_SOLO8, ROBOT_SOLO12, TASK_WALK, default_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "solorl.h")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


def test_header_declares_the_call_and_keeps_the_abi_version():
    hdr = open(HDR).read()
    assert re.search(r"#define SOLORL_ABI_VERSION 5\b", hdr)
    assert re.search(r"#define SOLORL_TERM_RULES 4\b", hdr)
    assert re.search(r"enum \{ SOLORL_TERM_HEIGHT = 1, SOLORL_TERM_TILT = 2, SOLORL_TERM_CONTACT = 4, SOLORL_TERM_JOINT = 8 \};", hdr)
    assert re.search(r"typedef struct solorl_termination \{.*?\} solorl_termination;", hdr, re.S)
    assert re.search(r"^int solorl_terminate\(const solorl_config\* cfg, const solorl_termination\* p,", hdr, re.M)
    assert re.search(r"^ \*   solorl_terminate +<-", hdr, re.M)                 # the opening list
    for piece in ("up_z = 1 - 2 (qx qx + qy qy)", "lambda_prev[p] / sim_dt", "timestep < min_steps", "fired_out[i] = 0, nothing else is written",
                  "reward[i] = (float)terminal_reward", "[2] += (float)timestep", "[4 + k] += (float)dr[k]", "masked (mask byte 0)",
                  "solorl_get_states -> solorl_terminate -> solorl_reset_masked"):
        assert piece in hdr, piece


def test_library_exports_and_binding(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert "solorl_terminate" in exported and "solorl_terminate" in _native.SYMBOLS
    assert lib.solorl_terminate.restype is C.c_int and len(lib.solorl_terminate.argtypes) == 12
    assert lib.solorl_abi_version() == 5                     # no existing struct changed


def test_ctypes_struct_equals_the_c_struct(tmp_path):
    """sizeof and every offset, from a program the host compiler builds against the header"""
    names = [n for n, _ in _native.Termination._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "solorl.h"\nint main(void) {\n  printf("%zu", sizeof(solorl_termination));\n'
                   + "".join('  printf(" %%zu", offsetof(solorl_termination, %s));\n' % n for n in names) + '  printf(" %d\\n", SOLORL_TERM_RULES);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = _native.Termination
    assert got == [C.sizeof(T)] + [getattr(T, n).offset for n in names] + [_native.TERM_RULES]
    assert C.sizeof(T) == 16 + 3 * 8 + 24 * 8 + 8 == 240 and termination.STAT_FIELDS == 5 and len(termination.RULES) == 4
    assert (termination.HEIGHT, termination.TILT, termination.CONTACT, termination.JOINT) == (1, 2, 4, 8)


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """Every refused argument returns SOLORL_ERR_INVALID with the function's name in front -- on a machine without a GPU too, so the
    check precedes the first HIP call (which would answer SOLORL_ERR_NODEVICE there)"""
    x = C.c_void_p(4096)
    nan, inf = float("nan"), float("inf")

    def call(robot=ROBOT_SOLO12, cfg=True, p=True, states=x, done=x, reward=x, fired=x, n=4, device=0, sim_dt=None, cfg_robot=None, **fields):
        c = default_config(robot, TASK_WALK)
        if sim_dt is not None:
            c.sim_dt = sim_dt
        if cfg_robot is not None:
            c.robot = cfg_robot
        P = termination.make_termination(robot, base_height=0.1, max_tilt_deg=60, contacts=["base", "knees"], contact_force_min=1.0,
                                         joint_limits=[-2.0, 2.0], min_steps=2)
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(P, v[0])[v[1]] = v[2]
            else:
                setattr(P, k, v)
        return lib.solorl_terminate(C.byref(c) if cfg else None, C.byref(P) if p else None, states, None, n, done, reward, fired, None, None, device, None)

    def refused(**kw):
        assert call(**kw) == -1, kw
        assert lib.solorl_last_error().startswith(b"solorl_terminate:"), lib.solorl_last_error()

    cases = [dict(cfg=False), dict(p=False), dict(states=None), dict(done=None), dict(reward=None), dict(fired=None), dict(n=0), dict(n=-5),
             dict(cfg_robot=2), dict(cfg_robot=-1), dict(sim_dt=0.0), dict(sim_dt=-1e-3), dict(sim_dt=nan), dict(sim_dt=inf),
             dict(rules=0), dict(rules=16), dict(rules=1 | 32), dict(rules=2 ** 31), dict(min_steps=-1),
             dict(min_height=nan), dict(min_height=inf), dict(min_up_z=nan), dict(min_up_z=-inf), dict(contact_force_min=nan),
             dict(contact_force_min=inf), dict(contact_force_min=-0.5), dict(rules=1, contact_force_min=-0.5),
             dict(terminal_reward=nan), dict(terminal_reward=-inf), dict(contact_prims=1 << 24), dict(contact_prims=1 << 31),
             dict(robot=ROBOT_SOLO8, contact_prims=1 << 20), dict(robot=ROBOT_SOLO8, contact_prims=1 << 23)]
    for robot, nq in ((ROBOT_SOLO12, 12), (ROBOT_SOLO8, 8)):
        for j in (0, nq - 1):
            cases += [dict(robot=robot, a=("joint_lo", j, nan)), dict(robot=robot, a=("joint_hi", j, inf)), dict(robot=robot, a=("joint_lo", j, 3.0)),
                      dict(robot=robot, rules=1, a=("joint_lo", j, 3.0))]
    for kw in cases:
        refused(**kw)
    # what is allowed passes the checks: what answers is the device check (a device id no machine has), before any launch
    for kw in (dict(), dict(robot=ROBOT_SOLO8), dict(rules=1, min_up_z=nan, contact_force_min=inf, a=("joint_hi", 0, inf)),
               dict(rules=8, min_height=nan, contact_prims=1 << 31), dict(robot=ROBOT_SOLO8, a=("joint_lo", 8, 3.0)),
               dict(robot=ROBOT_SOLO8, rules=3, contact_prims=1 << 22), dict(min_steps=2 ** 31 - 1), dict(n=1)):
        assert call(device=2 ** 20, **kw) == -2, (kw, lib.solorl_last_error())


def test_make_termination_reads_the_keys_and_refuses_unknown_ones_by_name():
    p = termination.make_termination(ROBOT_SOLO12, base_height=0.12, max_tilt_deg=60, contacts=["base", "shoulders", 14], contact_force_min=2.0,
                                     joint_limits=[-1.0, 2.0], min_steps=3, terminal_reward=-4.0)
    assert p.rules == 15 and p.min_steps == 3 and p.contact_prims == 0xFFF | (0xF << 20) | (1 << 14)
    assert (p.min_height, p.min_up_z, p.contact_force_min, p.terminal_reward) == (0.12, math.cos(math.radians(60.0)), 2.0, -4.0)
    assert list(p.joint_lo) == [-1.0] * 12 and list(p.joint_hi) == [2.0] * 12
    q = termination.make_termination(default_config(ROBOT_SOLO8, TASK_WALK), contacts="knees", joint_limits=[[-1.0 - j, 1.0 + j] for j in range(8)])
    assert q.rules == 4 | 8 and q.contact_prims == 0x55000 and q.terminal_reward == -10.0 and q.min_steps == 0 and q.contact_force_min == 0.0
    assert list(q.joint_hi) == [1.0 + j for j in range(8)] + [0.0] * 4
    assert termination.make_termination(ROBOT_SOLO12, base_height=0.05).rules == 1            # a rule is enabled by naming its key
    with pytest.raises(ValueError, match="max_tilt"):
        termination.make_termination(ROBOT_SOLO12, base_height=0.1, max_tilt=60)
    with pytest.raises(ValueError, match="heading"):
        termination.rules_from_dict({"base_height": 0.1, "heading": 1.0})
    for bad in (dict(), dict(min_steps=2), dict(contacts=["hips"]), dict(contacts=[24]), dict(contacts=[]), dict(contacts=[1.5]),
                dict(base_height=0.1, min_steps=-1), dict(base_height=0.1, min_steps=1.5), dict(max_tilt_deg=181), dict(max_tilt_deg=-1),
                dict(base_height=float("nan")), dict(base_height=0.1, terminal_reward=float("inf")), dict(joint_limits=[1.0, -1.0]),
                dict(joint_limits=[[0, 1]] * 8), dict(joint_limits=[0.0, float("inf")]), dict(base_height=0.1, contact_force_min=1.0),
                dict(contacts=["base"], contact_force_min=-1.0)):
        with pytest.raises(ValueError):
            termination.make_termination(ROBOT_SOLO12, **bad)
    with pytest.raises(ValueError, match="shoulders"):
        termination.make_termination(ROBOT_SOLO8, contacts=["shoulders"])                      # Solo12 only


def test_kernel_resources(lib):
    """The code-object metadata of both instantiations: the staged rows' static LDS, no scratch, no spills, no AGPRs, and few enough
    registers for eight wavefronts per SIMD -- LDS decides the residency, six workgroups per CU"""
    from solorl_amd import devcode
    res = {k: v for k, v in devcode.kernel_resources(build.LIB).items() if "term_rows_kernel" in k}
    assert len(res) == 2, sorted(res)
    for k, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 64 * (49 * 8 + 4) == 25344, (k, r)
        assert r.get("agpr_count", 0) == 0 and r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (k, r)
        assert r["vgpr_count"] <= 64, (k, r)
        assert (160 * 1024) // r["group_segment_fixed_size"] == 6


def test_launchers_parse_the_new_flag():
    sys.path.insert(0, ROOT)
    import train_ppo
    assert train_ppo.get_ppo_args([]).termination is None                        # default: off
    path = os.path.join(ROOT, "configs", "termination_walk12.yaml")
    assert train_ppo.get_ppo_args(["--termination", path]).termination == path
    out = subprocess.run([sys.executable, os.path.join(ROOT, "eval_ppo.py"), "--help"], capture_output=True, text=True, check=True).stdout
    assert "--termination" in out


def test_example_file_and_defaults(tmp_path):
    sys.path.insert(0, ROOT)
    import train_ppo
    from solorl_amd.config import load_yaml
    from solorl_amd.vec_env import SoloVecEnv, make_vec_envs
    path = os.path.join(ROOT, "configs", "termination_walk12.yaml")
    assert "UNTUNED" in open(path).read()
    config = load_yaml(os.path.join(ROOT, "configs", "basic12.yaml"))
    d = train_ppo.load_termination(path, config)
    p = termination.make_termination(ROBOT_SOLO12, **d)
    assert p.rules == termination.TILT | termination.CONTACT and p.contact_prims == 0xFFF | (0xF << 20) and p.min_steps == 2
    assert p.min_up_z == math.cos(math.radians(60.0)) and p.terminal_reward == -10.0
    bad = tmp_path / "bad.yaml"
    bad.write_text("base_height: 0.1\nmax_tilt: 60\n")
    with pytest.raises(SystemExit, match="max_tilt"):
        train_ppo.main(["--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--termination", str(bad)])
    with pytest.raises(SystemExit, match="shoulders"):                            # the example names Solo12 primitives
        train_ppo.load_termination(path, load_yaml(os.path.join(ROOT, "configs", "basic.yaml")))
    assert inspect.signature(make_vec_envs).parameters["termination"].default is None
    assert "set_termination" in dir(SoloVecEnv)
