"""Non-finite states through the kernel's sub-step code on the CPU, under the sanitizers (tests/host/nonfinite_main.cpp).

The step kernels promise (include/solorl.h) that a NaN/Inf state is no error: the env is force-terminated and reset.  On the way there
the poisoned values run through four sub-steps of collision, dynamics and PGS code.  This builds that code -- the same templates the HIP
kernels instantiate, compiled for one lane -- into a stand-alone program with AddressSanitizer and UBSan (float-cast-overflow
included), runs it as a child process and requires: no report (exit 0: -fno-sanitize-recover=all aborts at the first one), and the
guard's sum non-finite or beyond its threshold on every line whose state is.  tests/test_nan_guard_gpu.py runs the same poisons on
the device."""
import shutil
from concurrent.futures import ThreadPoolExecutor

import pytest

from solorl_amd.config import default_config, ROBOT_SOLO8, ROBOT_SOLO12, TASK_WALK
from tests.host_util import build_host, run_host, san_flags, sanitizers_link

POISONS = ("action_nan", "lin_vel_z_inf", "q_nan", "quat_x_nan", "pos_x_1e31", "pos_z_nan", "pos_y_nan", "ang_vel_neg_inf")


def test_nonfinite_states_under_the_sanitizers(tmp_path):
    if shutil.which("g++") is None or not sanitizers_link():
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    # the four instantiations (robot x arithmetic type) as four programs, compiled side by side
    variants = [(robot, use_float) for robot in (ROBOT_SOLO12, ROBOT_SOLO8) for use_float in (1, 0)]
    with ThreadPoolExecutor(len(variants)) as pool:
        exes = list(pool.map(lambda v: build_host("nonfinite_main", san_flags("nonfinite_main") + ["-DHARNESS_ONLY_ROBOT=%d" % v[0], "-DHARNESS_ONLY_FLOAT=%d" % v[1]],
                                                  tmp_path), variants))
    lines = []
    for (robot, _), exe in zip(variants, exes):
        cfg = str(tmp_path / ("cfg%d.bin" % robot))
        with open(cfg, "wb") as f:
            f.write(bytes(default_config(robot, TASK_WALK)))
        lines += [l.split() for l in run_host(exe, (cfg,)).splitlines() if l.startswith("robot ")]
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
