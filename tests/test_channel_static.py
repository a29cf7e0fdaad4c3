"""Static checks of solorl_obs_noise and solorl_actuate (no GPU): the library exports both and _native binds them, the Python mirrors of
solorl_actuation and solorl_env_actuator agree with the header, which still has ABI version 5 and holds both draw tables; every argument
the entry points must refuse is refused before any HIP call; the three kernels use no LDS, no scratch, no AGPRs, no FLAT access and no
atomics; train_ppo.py and eval_ppo.py parse the three flags and make_vec_envs leaves everything off by default."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import pytest

from solorl_amd import _native, build, channel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


def test_library_exports_and_binding(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for n in ("solorl_obs_noise", "solorl_actuate"):
        assert n in exported and n in _native.SYMBOLS and getattr(lib, n).restype is C.c_int and getattr(lib, n).argtypes
    assert len(lib.solorl_obs_noise.argtypes) == 11 and len(lib.solorl_actuate.argtypes) == 8
    assert lib.solorl_abi_version() == 5                     # no existing struct changed


def test_python_mirrors_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "solorl.h")).read()
    assert re.search(r"#define SOLORL_ABI_VERSION 5\b", hdr)
    assert int(re.search(r"#define SOLORL_DELAY_MAX (\d+)", hdr).group(1)) == _native.DELAY_MAX == 4
    assert C.sizeof(_native.EnvActuator) == 256 == channel.ROW_BYTES and channel.ROW_WORDS == 64
    assert C.sizeof(_native.Actuation) == 40
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
                    dims = tuple(4 if x == "SOLORL_DELAY_MAX" else int(x) for x in re.findall(r"\[(\w+)\]", m.group(2)))
                    out.append((m.group(1), ctypes_of[ctype], dims))
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
    assert members("solorl_actuation") == mirror(_native.Actuation)
    assert members("solorl_env_actuator") == mirror(_native.EnvActuator)
    E = _native.EnvActuator
    assert (E.buf.offset, E.gain.offset, E.latency.offset, E.fill.offset, E.episodes.offset) == (0, 192, 240, 244, 248)
    # both draw tables and the opening list
    for piece in ("(gid_lo, gid_hi, block, 5)", "count[i] * B + b", "(gid_lo, gid_hi, 4 e, 6)", "4 e + 1 + j / 4", "(word >> 8) * 2^-24",
                  "delay_min + word % (delay_max - delay_min + 1)", "buf[min(latency, fill) - 1][j]", "min(fill + 1, delay_max)"):
        assert piece in hdr, piece
    assert re.search(r"^ \*   solorl_obs_noise / solorl_actuate :", hdr, re.M)
    mem = channel.ActuatorMem(3, "cpu")
    assert mem.data.shape == (3, 64) and mem.buf.shape == (3, 4, 12) and mem.gain.shape == (3, 12)
    mem.buf[1, 2, 5] = 1.5; mem.gain[2, 11] = 2.5; mem.latency[0] = 3; mem.fill[1] = 2; mem.episodes[2] = 7
    ints = mem.data.view(__import__("torch").int32)
    assert mem.data[1, 2 * 12 + 5] == 1.5 and mem.data[2, 59] == 2.5 and ints[0, 60] == 3 and ints[1, 61] == 2 and ints[2, 62] == 7


def test_bad_arguments_are_refused_before_any_hip_call(lib):
    """Every refused argument returns SOLORL_ERR_INVALID with the function's name in front -- on a machine without a GPU too, so the
    check precedes the first HIP call (which would answer SOLORL_ERR_NODEVICE there)"""
    x = C.c_void_p(4096)

    def noise(scale=x, count=x, obs_in=x, obs_out=x, n=4, D=76):
        assert lib.solorl_obs_noise(1, 0, scale, None, n, D, count, obs_in, obs_out, 0, None) == -1
        assert lib.solorl_last_error().startswith(b"solorl_obs_noise:"), lib.solorl_last_error()

    for kw in (dict(scale=None), dict(count=None), dict(obs_in=None), dict(obs_out=None), dict(n=0), dict(n=-2), dict(D=0), dict(D=-1), dict(D=211),
               dict(D=2 ** 31 - 1)):
        noise(**kw)

    def act(p=True, mem=x, a_in=x, a_out=x, n=4, **fields):
        P = _native.Actuation(1, 0, 12, 0, 3, 0, 0.2)
        for k, v in fields.items():
            setattr(P, k, v)
        assert lib.solorl_actuate(C.byref(P) if p else None, n, None, mem, a_in, a_out, 0, None) == -1
        assert lib.solorl_last_error().startswith(b"solorl_actuate:"), lib.solorl_last_error()

    for kw in (dict(p=False), dict(mem=None), dict(a_in=None), dict(a_out=None), dict(n=0), dict(n=-1), dict(act_dim=0), dict(act_dim=10), dict(act_dim=16),
               dict(delay_min=-1), dict(delay_min=4), dict(delay_max=5), dict(delay_min=2, delay_max=1), dict(gain_range=-0.1), dict(gain_range=1.0),
               dict(gain_range=float("nan")), dict(gain_range=float("inf")), dict(gain_range=-float("inf"))):
        act(**kw)


def test_kernels_use_no_lds_no_scratch_and_no_atomics(lib):
    """Both kernels are a load, a Philox block and a store per thread: everything stays in registers, memory is reached through global
    instructions only, and the counter update of the noise kernel is a plain store behind the workgroup's barrier"""
    from solorl_amd import devcode
    res = {k: v for k, v in devcode.kernel_resources(build.LIB).items() if "obs_noise_kernel" in k or "actuate_kernel" in k}
    assert len(res) == 3 and sum("obs_noise_kernelILb1" in k for k in res) == 1 and sum("obs_noise_kernelILb0" in k for k in res) == 1, sorted(res)
    for k, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, (k, r)
        assert r.get("agpr_count", 0) == 0 and r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, (k, r)
        assert r["vgpr_count"] <= 64, (k, r)                 # eight wavefronts per SIMD
    st = devcode.function_stats(build.LIB)
    for k in res:
        assert st[k]["scratch"] == 0 and st[k]["flat"] == 0 and st[k]["global"] > 0, (k, st[k])
        assert st[k]["barriers"] == (1 if "obs_noise" in k else 0), (k, st[k])
    text, cur, ops = devcode.disassemble(build.LIB), None, {k: [] for k in res}
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = ops.get(m.group(1))
        elif cur is not None and "\t" in line:
            cur.append(line.split("\t")[1].strip().split(" ")[0])
    for k, o in ops.items():
        assert o and not [x for x in o if "atomic" in x], (k, [x for x in o if "atomic" in x])
        if "obs_noise_kernelILb1" in k:                      # the 16-byte path moves rows as 16-byte words
            assert "global_load_dwordx4" in o and "global_store_dwordx4" in o, k
        assert not [x for x in o if x.startswith("v_fma_f64") or x.startswith("v_fmac_f64")], k      # every product and sum rounds on its own


def test_launchers_parse_the_three_flags():
    sys.path.insert(0, ROOT)
    import train_ppo
    a = train_ppo.get_ppo_args([])
    assert a.obs_noise is None and a.action_delay is None and a.motor_gain_range == 0.0          # default: off
    path = os.path.join(ROOT, "configs", "noise_solo.yaml")
    a = train_ppo.get_ppo_args(["--obs-noise", path, "--action-delay", "1:3", "--motor-gain-range", "0.2"])
    assert a.obs_noise == path and a.action_delay == (1, 3) and a.motor_gain_range == 0.2
    assert train_ppo.get_ppo_args(["--action-delay", "2"]).action_delay == (2, 2)
    assert train_ppo.get_ppo_args(["--action-delay", "0:4"]).action_delay == (0, 4)
    for bad in ("-1", "3:2", "0:5", "a", "1:2:3", ""):
        with pytest.raises(SystemExit):
            train_ppo.get_ppo_args(["--action-delay", bad])
    for bad in ("-0.1", "1.0", "x"):
        with pytest.raises(SystemExit):
            train_ppo.get_ppo_args(["--motor-gain-range", bad])
    # eval_ppo.py takes the same flags (its parser is built inside main: read them from its --help)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "eval_ppo.py"), "--help"], capture_output=True, text=True, check=True).stdout
    for flag in ("--obs-noise", "--action-delay", "--motor-gain-range"):
        assert flag in out, flag


def test_example_file_and_defaults(tmp_path):
    import yaml
    sys.path.insert(0, ROOT)
    import train_ppo
    from solorl_amd.config import config_from_dict, load_yaml
    from solorl_amd.vec_env import make_vec_envs
    path = os.path.join(ROOT, "configs", "noise_solo.yaml")
    assert "UNTUNED" in open(path).read()
    d = yaml.safe_load(open(path))
    for cfgfile in ("basic.yaml", "basic12.yaml"):
        cfg = config_from_dict(load_yaml(os.path.join(ROOT, "configs", cfgfile)))
        v = channel.scales_from_dict(cfg, d)
        assert tuple(v.shape) == (cfg.obs_dim,) and int((v > 0).sum()) >= 2 * (10 + 2 * cfg.n_joints)
        assert float(v[10 + 2 * cfg.n_joints:14 + 2 * cfg.n_joints].abs().sum()) == 0.0      # the feet flags
    bad = tmp_path / "bad.yaml"
    bad.write_text("groups:\n  hieght: 0.1\n")
    with pytest.raises(SystemExit, match="hieght"):
        train_ppo.main(["--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--obs-noise", str(bad)])
    p = inspect.signature(make_vec_envs).parameters
    assert p["obs_noise"].default is None and p["action_delay"].default is None and p["motor_gain_range"].default == 0.0
