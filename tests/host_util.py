"""Shared by the tests that run the engine's host-and-device code on the CPU: the stand-alone programs of tests/host built by g++ and run
as child processes, the bit-pattern helpers of their text protocols, and the Philox block every draw table of include/solorl.h starts
from.  Each program's protocol and reference model stay with its own ``*_util.py``."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile
import zlib

import numpy as np

from oracle import oracle_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
M32 = 0xFFFFFFFF

# the two sanitizer sets the programs are built with
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SAN_FLOAT = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]

# program (tests/host/<program>.cpp) -> (its fixed compiler flags, the sanitizer set it takes).  No -march=native anywhere; with
# -ffp-contract=off every operation rounds on its own.  The rows are each program's own: they are not meant to agree.
PROGRAMS = {
    "perturb_main": (["-Wall", "-Werror"], SAN_FLOAT),
    "channel_main": (["-Wall", "-Werror", "-ffp-contract=off"], SAN),
    "terminate_main": (["-Wall", "-Werror", "-ffp-contract=off"], SAN),
    "command_main": (["-Wall", "-Werror", "-ffp-contract=off", "-DSOLO_HOST_SHIM"], SAN),
    "rows_main": (["-DSOLO_HOST_SHIM", "-I" + HOST], SAN),
    "shape_main": (["-DSOLO_HOST_SHIM", "-I" + HOST], SAN),
    "reset_random_main": (["-DSOLO_HOST_SHIM", "-I" + HOST, "-ffp-contract=off"], SAN),
    "nonfinite_main": (["-I" + HOST], SAN_FLOAT),
}


# ---------------------------------------------------------------- building and running
def _cxx():
    cxx = shutil.which("g++")
    assert cxx is not None, "no g++"
    return cxx


@functools.lru_cache(maxsize=None)
def _tmp():
    d = tempfile.mkdtemp(prefix="solorl_host_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


@functools.lru_cache(maxsize=None)
def sanitizers_link():
    """can g++ link the sanitizer runtimes here (and a program built with them start)"""
    src, exe = os.path.join(_tmp(), "probe.cpp"), os.path.join(_tmp(), "probe")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run([_cxx(), *SAN_FLOAT, "-o", exe, src], capture_output=True)
    return r.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0


def san_flags(program):
    """the sanitizer flags ``program`` is built with"""
    return PROGRAMS[program][1]


_BUILT = {}


def build_host(program, flags=(), out_dir=None):
    """tests/host/<program>.cpp -> an executable built by g++ with the program's fixed flags and ``flags`` (san_flags(program), -D switches),
    once per process and set of flags; in ``out_dir`` or a directory that lives as long as the process"""
    key = (program, tuple(flags))
    if key not in _BUILT:
        fixed, _ = PROGRAMS[program]
        exe = os.path.join(str(out_dir) if out_dir is not None else _tmp(), "%s_%08x" % (program, zlib.crc32(" ".join(flags).encode())))
        # (-g1: file and line in a sanitizer report; full -g more than doubles the build time and adds nothing to a check)
        cmd = [_cxx(), "-O1", "-g1", "-std=c++17"] + fixed + list(flags) + ["-o", exe, os.path.join(HOST, program + ".cpp")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        _BUILT[key] = exe
    return _BUILT[key]


def run_host(exe, args=(), input=None, timeout=300):
    """The program as a child process -> its standard output; it must exit 0 (-fno-sanitize-recover=all aborts at the first report)
    and leave no sanitizer report"""
    r = subprocess.run([exe, *args], input=input, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


# ---------------------------------------------------------------- bit patterns (a bitwise comparison tells -0.0 from +0.0 and compares NaNs)
def bits32(x):
    """float32 array -> its bit patterns (uint32)"""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def bits64(x):
    """float64 array -> its bit patterns (uint64)"""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def hex32(x):
    """float32 values -> their words in hexadecimal, separated by blanks"""
    return " ".join("%08x" % int(w) for w in bits32(x).reshape(-1))


def hex64(x):
    """float64 values -> their words in hexadecimal, separated by blanks"""
    return " ".join("%016x" % int(w) for w in bits64(x).reshape(-1))


# ---------------------------------------------------------------- the draws
def philox_block(seed, gid, block, stream):
    """the four words of key (seed_lo, seed_hi), counter (gid_lo, gid_hi, block mod 2^32, stream), by the oracle's Philox"""
    return oracle_py.philox(seed & M32, (seed >> 32) & M32, gid & M32, (gid >> 32) & M32, block & M32, stream)


def u24(word):
    """u = (word >> 8) 2^-24 in [0, 1), exact in a double"""
    return float(word >> 8) * (1.0 / 16777216.0)
