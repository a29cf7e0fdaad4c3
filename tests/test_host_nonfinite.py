"""Non-finite states through the kernel's sub-step code on the CPU, under the sanitizers (tests/host/nonfinite_main.cpp).

The step kernels promise (include/solorl.h) that a NaN/Inf state is no error: the env is force-terminated and reset.  On the way there
the poisoned values run through four sub-steps of collision, dynamics and PGS code.  This builds that code -- the same templates the HIP
kernels instantiate, compiled for one lane -- into a stand-alone program with AddressSanitizer and UBSan (float-cast-overflow
included), runs it as a child process and requires: no report (exit 0: -fno-sanitize-recover=all aborts at the first one), and the
guard's sum non-finite or beyond its threshold on every line whose state is.  tests/test_nan_guard_gpu.py runs the same poisons on
the device."""
import os
import shutil
import subprocess

import pytest

from solorl_amd.config import default_config, ROBOT_SOLO8, ROBOT_SOLO12, TASK_WALK

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")
SAN = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]
POISONS = ("action_nan", "lin_vel_z_inf", "q_nan", "quat_x_nan", "pos_x_1e31", "pos_z_nan", "pos_y_nan", "ang_vel_neg_inf")


def _sanitizers_link(cxx, tmp):
    src = os.path.join(tmp, "probe.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    exe = os.path.join(tmp, "probe")
    r = subprocess.run([cxx, *SAN, "-o", exe, src], capture_output=True)
    return r.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0


def test_nonfinite_states_under_the_sanitizers(tmp_path):
    # (-g1: file and line in a sanitizer report; full -g more than doubles the four builds' time and adds nothing to the check)
    cxx = shutil.which("g++")
    if cxx is None or not _sanitizers_link(cxx, str(tmp_path)):
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    # the four instantiations (robot x arithmetic type) as four programs, compiled side by side
    builds = []
    for robot in (ROBOT_SOLO12, ROBOT_SOLO8):
        cfg = str(tmp_path / ("cfg%d.bin" % robot))
        with open(cfg, "wb") as f:
            f.write(bytes(default_config(robot, TASK_WALK)))
        for use_float in (1, 0):
            exe = str(tmp_path / ("nonfinite_r%d_f%d" % (robot, use_float)))
            cmd = [cxx, "-O1", "-g1", "-std=c++17", *SAN, "-DHARNESS_ONLY_ROBOT=%d" % robot, "-DHARNESS_ONLY_FLOAT=%d" % use_float, "-I" + HERE,
                   "-o", exe, os.path.join(HERE, "nonfinite_main.cpp")]
            builds.append((subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), exe, cfg))
    lines = []
    for proc, exe, cfg in builds:
        out, _ = proc.communicate()
        assert proc.returncode == 0, out[-4000:]
    for proc, exe, cfg in builds:
        r = subprocess.run([exe, cfg], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-4000:]
        lines += [l.split() for l in r.stdout.splitlines() if l.startswith("robot ")]
    # robot x {float, double} x treadmill {0, 1} x the poisons (pos_y_nan: with the treadmill only)
    assert len(lines) == 2 * 2 * (2 * len(POISONS) - 1), len(lines)
    seen = set()
    for w in lines:
        name, state, guard = w[w.index("poison") + 1], w[w.index("state") + 1], w[w.index("guard") + 1]
        seen.add((name, w[1], w[2]))
        assert int(w[w.index("contacts") + 1], 16) & 0xFFFFFF, w       # the poisoned sub-steps had constraint rows to go through
        assert state == "bad", w                    # every poison leaves at least its own component non-finite / beyond 1e30
        assert guard == "fires", w
    assert seen == {(p, r, t) for p in POISONS for r in ("0", "1") for t in ("float", "double")}
