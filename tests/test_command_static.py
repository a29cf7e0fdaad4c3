"""Static checks of solorl_commands and solorl_shape_reward_cmd (no GPU): the library exports both and _native binds them, the Python
mirrors of solorl_command_params and solorl_env_command agree with the header, which still has ABI version 5 and holds the draw table;
every argument solorl_commands must refuse is refused before any HIP call; the kernel uses no LDS and no scratch; train_ppo.py and
eval_ppo.py parse the new flags, the example file loads and make_vec_envs leaves commands off by default."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import pytest

from solorl_amd import _native, build, command

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


def test_library_exports_and_binding(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for n in ("solorl_commands", "solorl_shape_reward_cmd"):
        assert n in exported and n in _native.SYMBOLS and getattr(lib, n).restype is C.c_int and getattr(lib, n).argtypes
    assert len(lib.solorl_commands.argtypes) == 10
    assert len(lib.solorl_shape_reward_cmd.argtypes) == len(lib.solorl_shape_reward.argtypes) + 1 == 14
    assert lib.solorl_abi_version() == 5                     # no existing struct changed


def test_python_mirrors_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "solorl.h")).read()
    assert re.search(r"#define SOLORL_ABI_VERSION 5\b", hdr)
    assert C.sizeof(_native.EnvCommand) == 32 == command.ROW_BYTES and command.ROW_WORDS == 4
    assert C.sizeof(_native.CommandParams) == 2 * 8 + 11 * 8 + 4 * 4 == 120
    ctypes_of = {"uint64_t": C.c_uint64, "int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "double": C.c_double, "float": C.c_float}

    def members(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for stmt in body.split(";"):
            stmt = stmt.strip()
            if stmt:
                ctype, rest = stmt.split(None, 1)
                for d in rest.split(","):
                    m = re.match(r"\s*(\w+)((?:\[\w+\])*)\s*$", d)
                    out.append((m.group(1), ctypes_of[ctype], tuple(int(x) for x in re.findall(r"\[(\w+)\]", m.group(2)))))
        return out

    def mirror(cls):
        out = []
        for n, t in cls._fields_:
            dims = []
            while hasattr(t, "_length_"):
                dims.append(t._length_)
                t = t._type_
            out.append((n, t, tuple(dims)))
        return out
    assert members("solorl_command_params") == mirror(_native.CommandParams)
    assert members("solorl_env_command") == mirror(_native.EnvCommand)
    E, P = _native.EnvCommand, _native.CommandParams
    assert (E.cmd.offset, E.countdown.offset, E.draws.offset) == (0, 24, 28)
    assert (P.seed.offset, P.env_id_offset.offset, P.lo.offset, P.hi.offset, P.obs_scale.offset, P.zero_prob.offset, P.min_lin_norm.offset,
            P.interval_min.offset, P.interval_max.offset, P.obs_dim.offset, P.reserved.offset) == (0, 8, 16, 40, 64, 88, 96, 104, 108, 112, 116)
    # the draw table and the opening list
    for piece in ("(gid_lo, gid_hi, 2 d, 7)", "(gid_lo, gid_hi, 2 d + 1, 7)", "interval_min + word % (interval_max - interval_min + 1)",
                  "(word >> 8) * 2^-24", "lo_k + u_k * (hi_k - lo_k)", "u < zero_prob", "min_lin_norm * min_lin_norm",
                  "(float)(cmd_k * obs_scale[k])", "mem.draws == 0"):
        assert piece in hdr, piece
    assert re.search(r"^ \*   solorl_commands / solorl_shape_reward_cmd :", hdr, re.M)
    mem = command.CommandMem(3, "cpu")
    assert mem.data.shape == (3, 4) and mem.cmd.shape == (3, 3)
    mem.cmd[1, 2] = 1.5; mem.countdown[0] = 3; mem.draws[2] = 7
    ints = mem.data.view(__import__("torch").int32)
    assert mem.data[1, 2] == 1.5 and ints[0, 6] == 3 and ints[2, 7] == 7


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """Every refused argument returns SOLORL_ERR_INVALID with the function's name in front -- on a machine without a GPU too, so the
    check precedes the first HIP call (which would answer SOLORL_ERR_NODEVICE there)"""
    x = C.c_void_p(4096)
    nan, inf = float("nan"), float("inf")

    def refused(p=True, mem=x, obs_in=x, obs_out=x, n=4, **fields):
        P = command.make_params(1, 0, 76, lin_vel_x=(-1.0, 1.0), lin_vel_y=(-0.5, 0.5), yaw_rate=(-1.0, 1.0), interval=(2, 5), zero_prob=0.1,
                                min_lin_norm=0.2)
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(P, v[0])[v[1]] = v[2]
            else:
                setattr(P, k, v)
        assert lib.solorl_commands(C.byref(P) if p else None, None, None, n, mem, obs_in, obs_out, None, 0, None) == -1, (fields, n)
        assert lib.solorl_last_error().startswith(b"solorl_commands:"), lib.solorl_last_error()

    cases = [dict(p=False), dict(mem=None), dict(obs_in=None), dict(obs_out=None), dict(n=0), dict(n=-3), dict(obs_dim=0), dict(obs_dim=-1),
             dict(obs_dim=211), dict(obs_dim=2 ** 31 - 1), dict(zero_prob=-0.01), dict(zero_prob=1.01), dict(zero_prob=nan),
             dict(min_lin_norm=-0.1), dict(min_lin_norm=nan), dict(min_lin_norm=inf), dict(interval_min=0), dict(interval_min=-1),
             dict(interval_min=6), dict(interval_max=(1 << 20) + 1), dict(interval_min=3, interval_max=2)]
    for k in range(3):
        cases += [dict(a=("lo", k, nan)), dict(a=("hi", k, nan)), dict(a=("lo", k, -inf)), dict(a=("hi", k, inf)), dict(a=("lo", k, 2.0)),
                  dict(a=("obs_scale", k, nan)), dict(a=("obs_scale", k, inf))]
    for kw in cases:
        refused(**kw)
    # parameters at the edges of what is allowed pass: what answers is the device check (a device id no machine has), before any launch
    P = command.make_params(1, 0, 210, lin_vel_x=(-1.0, 1.0), interval=(1, 1 << 20), zero_prob=1.0)
    assert lib.solorl_commands(C.byref(P), None, None, 1, x, None, None, None, 2 ** 20, None) == -2, lib.solorl_last_error()
    # solorl_shape_reward_cmd refuses what solorl_shape_reward refuses, under its prefix
    assert lib.solorl_shape_reward_cmd(None, None, None, None, 0, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.solorl_last_error().startswith(b"solorl_shape_reward:"), lib.solorl_last_error()


def test_python_side_refusals():
    for bad in (dict(lin_vel_x=(1.0, -1.0)), dict(yaw_rate=(0.0, float("inf"))), dict(interval=0), dict(interval=(3, 2)), dict(interval=1.5),
                dict(zero_prob=1.5), dict(min_lin_norm=-1.0), dict(obs_scale=(1.0, 2.0)), dict(heading=(0.0, 1.0))):
        with pytest.raises(ValueError):
            command.make_params(1, 0, 76, **bad)
    with pytest.raises(ValueError, match="lin_vel_z"):
        command.ranges_from_dict({"lin_vel_z": [0, 1]})
    p = command.make_params(2 ** 64 + 5, 7, 42, lin_vel_x=0.3, interval=4)
    assert (p.seed, p.env_id_offset, p.obs_dim, p.lo[0], p.hi[0], p.interval_min, p.interval_max) == (5, 7, 42, 0.3, 0.3, 4, 4)
    assert list(p.obs_scale) == [1.0, 1.0, 1.0] and p.zero_prob == 0.0
    q = command.make_params(5, 7, 42, **dict(command.ranges_of(p), yaw_rate=(-1.0, 1.0)))
    assert (q.lo[0], q.hi[0], q.lo[2], q.hi[2], q.interval_min) == (0.3, 0.3, -1.0, 1.0, 4)


def test_kernel_uses_no_lds_and_no_scratch(lib):
    """The code-object metadata of both instantiations (obs_in read as 16-byte words, and word by word): no LDS, no scratch, no
    spills, and few enough registers for eight wavefronts per SIMD"""
    from solorl_amd import devcode
    res = {k: v for k, v in devcode.kernel_resources(build.LIB).items() if "command_kernel" in k}
    assert len(res) == 2 and sum("command_kernelILb1" in k for k in res) == 1 and sum("command_kernelILb0" in k for k in res) == 1, sorted(res)
    for k, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, (k, r)
        assert r.get("agpr_count", 0) == 0 and r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (k, r)
        assert r["vgpr_count"] <= 64, (k, r)
    lds = devcode.kernel_static_lds(build.LIB)
    assert all(lds[k] == 0 for k in res)


def test_launchers_parse_the_new_flags():
    sys.path.insert(0, ROOT)
    import train_ppo
    assert train_ppo.get_ppo_args([]).commands is None                           # default: off
    path = os.path.join(ROOT, "configs", "commands_walk12.yaml")
    assert train_ppo.get_ppo_args(["--commands", path]).commands == path
    out = subprocess.run([sys.executable, os.path.join(ROOT, "eval_ppo.py"), "--help"], capture_output=True, text=True, check=True).stdout
    assert "--commands" in out and "--command VX VY WZ" in out
    r = subprocess.run([sys.executable, os.path.join(ROOT, "eval_ppo.py"), "--checkpoint-dir", "x", "--command", "0.3", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--command" in r.stderr                       # three numbers


def test_example_file_and_defaults(tmp_path):
    sys.path.insert(0, ROOT)
    import train_ppo
    from solorl_amd.vec_env import SoloVecEnv, make_vec_envs
    path = os.path.join(ROOT, "configs", "commands_walk12.yaml")
    assert "UNTUNED" in open(path).read()
    d = train_ppo.load_commands(path)
    assert set(d) == set(command.KEYS)
    p = command.make_params(1, 0, 76, **d)
    assert all(p.lo[k] < 0.0 < p.hi[k] for k in range(3)) and 1 <= p.interval_min < p.interval_max and 0.0 < p.zero_prob < 1.0
    bad = tmp_path / "bad.yaml"
    bad.write_text("lin_vel_x: [0.0, 1.0]\nyaw_rat: [0.0, 1.0]\n")
    with pytest.raises(SystemExit, match="yaw_rat"):
        train_ppo.main(["--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--commands", str(bad)])
    assert inspect.signature(make_vec_envs).parameters["commands"].default is None
    assert inspect.signature(SoloVecEnv.__init__).parameters["commands"].default is None
