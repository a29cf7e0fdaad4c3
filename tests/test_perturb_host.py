"""Device-side kicks (include/solorl.h solorl_set_perturbation / solorl_perturb / solorl_get_perturbation) without a GPU.

The draw arithmetic of the kernel is solorl_amd/csrc/perturb.hpp, plain host-and-device functions: tests/host/perturb_main.cpp compiles
them with the host compiler into a stand-alone program (under AddressSanitizer and UBSan where g++ can link them, as the other programs
of tests/host are), and its first countdown and first four kicks of ~200 (seed, gid) pairs are compared with tests/perturb_util.py --
the oracle's Philox and the draw table of the header -- doubles bitwise, countdowns exactly.  Then the binding: the library exports the
three calls, _native binds them, the ctypes mirror has the struct's size, the perturb kernel exists for both arithmetic types without
scratch, and train_ppo.py parses --push-interval."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from solorl_amd import _native, build
from tests import perturb_util as pu
from tests.host_util import ROOT, build_host, hex64 as _hex, run_host, san_flags, sanitizers_link


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


def _cases():
    """~200 (seed, gid, interval, amplitudes): small and large seeds, gids above 2^32, the interval (1, 1), zero amplitudes"""
    rng = np.random.default_rng(17)
    seeds = [0, 1, 5, 2301, 0xFFFFFFFF, 0x123456789ABCDEF, 2 ** 64 - 1]
    gids = [0, 1, 3, 257, 65535, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 3 * 2 ** 32 + 11, 2 ** 40 + 12345, 2 ** 62 + 1]
    intervals = [(1, 1), (2, 5), (10, 20), (7, 7), (1, 1000), (3, 2 ** 31 - 1)]
    amps = [(0.5, 0.3, 0.2, 0.4, 0.6, 1.0), (0.5, 0.0, 0.0, 0.0, 0.0, 0.0), (0.0,) * 6, (0.5, 0.5, 0.0, 0.0, 0.0, 0.5), (1e-3, 7.25, 0.1, 1e6, 1e-300, 3.0)]
    out = []
    for k in range(200):
        out.append((seeds[k % len(seeds)] if k % 3 else int(rng.integers(0, 2 ** 63)), gids[k % len(gids)] if k % 4 else int(rng.integers(0, 2 ** 62)),
                    intervals[k % len(intervals)], amps[k % len(amps)]))
    return out


def test_host_program_draws_equal_the_python_prediction(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    # (where g++ cannot link the sanitizer runtimes, the plain program checks the same draws)
    exe = build_host("perturb_main", san_flags("perturb_main") if sanitizers_link() else (), tmp_path)
    cases = _cases()
    text = "".join("%d %d %d %d %s\n" % (s, g, lo, hi, _hex(amp)) for s, g, (lo, hi), amp in cases)
    lines = run_host(exe, input=text, timeout=120).splitlines()
    assert len(lines) == len(cases) >= 200
    kicked = 0
    for (seed, gid, (lo, hi), amp), line in zip(cases, lines):
        w = line.split()
        assert len(w) == 1 + 4 * 7
        assert int(w[0]) == pu.first_countdown(seed, gid, lo, hi), (seed, gid, lo, hi)
        assert lo <= int(w[0]) <= hi
        for j in range(4):
            want, nxt = pu.kick(seed, gid, j, lo, hi, amp)
            got = w[1 + 7 * j:8 + 7 * j]
            assert got[:6] == [_hex(x) for x in want], (seed, gid, j, amp)
            assert int(got[6]) == nxt and lo <= nxt <= hi, (seed, gid, j)
            for k in range(6):
                assert abs(want[k]) <= amp[k]
                if amp[k] == 0.0:
                    assert got[k] == "0" * 16                # +0.0, not -0.0
            kicked += int(np.count_nonzero(want))
    assert kicked > 2000                                     # (the comparison was not one of zeros)


def test_library_exports_and_binding(lib):
    names = ("solorl_set_perturbation", "solorl_perturb", "solorl_get_perturbation")
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for n in names:
        assert n in exported and n in _native.SYMBOLS and getattr(lib, n).restype is C.c_int and getattr(lib, n).argtypes
    assert C.sizeof(_native.Perturbation) == 56
    assert [f[0] for f in _native.Perturbation._fields_] == ["interval_min", "interval_max", "max_lin_vel", "max_ang_vel"]
    assert _native.Perturbation.max_lin_vel.offset == 8 and _native.Perturbation.max_ang_vel.offset == 32
    # the error convention: null handle -> SOLORL_ERR_INVALID, the message names the call
    assert lib.solorl_set_perturbation(None, None) == -1 and b"solorl_set_perturbation" in lib.solorl_last_error()
    assert lib.solorl_perturb(None, None, None) == -1 and b"solorl_perturb" in lib.solorl_last_error()
    assert lib.solorl_get_perturbation(None, None, None, None) == -1 and b"solorl_get_perturbation" in lib.solorl_last_error()
    assert lib.solorl_abi_version() == 5                     # no existing struct changed


def test_header_declares_the_struct_and_the_draw_table():
    h = open(os.path.join(ROOT, "include", "solorl.h")).read()
    assert re.search(r"typedef struct solorl_perturbation \{\s*int32_t interval_min, interval_max;[^}]*double\s+max_lin_vel\[3\];[^}]*double\s+max_ang_vel\[3\];", h)
    for piece in ("(gid_lo, gid_hi, block, 4)", "block 1 + 2 j", "block 2 + 2 j", "(word >> 8) * 2^-24", "interval_min + word % (interval_max - interval_min + 1)"):
        assert piece in h, piece


def test_perturb_kernel_exists_for_both_types_and_uses_no_scratch(lib):
    """One thread per env, six words of state: the kick's six doubles must stay in registers."""
    from solorl_amd import devcode
    res = devcode.kernel_resources(build.LIB)
    found = {}
    for k, v in res.items():
        m = re.search(r"\d+perturb_kernelI([fd])E", k)
        if m:
            found[m.group(1)] = v
    assert sorted(found) == ["d", "f"], sorted(res)
    for t, r in found.items():
        assert r["private_segment_fixed_size"] == 0, (t, r)
        assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (t, r)


def test_train_ppo_parses_the_push_flags():
    import train_ppo
    a = train_ppo.get_ppo_args([])
    assert a.push_interval is None and a.push_max_vel == 0.0 and a.push_max_yaw_rate == 0.0          # default: off
    assert train_ppo.get_ppo_args(["--push-interval", "5"]).push_interval == (5, 5)
    a = train_ppo.get_ppo_args(["--push-interval", "5:10", "--push-max-vel", "0.5", "--push-max-yaw-rate", "0.25"])
    assert a.push_interval == (5, 10) and a.push_max_vel == 0.5 and a.push_max_yaw_rate == 0.25
    for bad in ("0", "10:5", "a", "1:2:3", ""):
        with pytest.raises(SystemExit):
            train_ppo.get_ppo_args(["--push-interval", bad])


def test_make_vec_envs_defaults_leave_the_perturbation_off():
    import inspect
    from solorl_amd.vec_env import make_vec_envs
    p = inspect.signature(make_vec_envs).parameters
    assert p["push_interval"].default is None and p["push_max_vel"].default == 0.0 and p["push_max_yaw_rate"].default == 0.0
