"""Time-limit bootstrapping without a GPU: the storage's CPU formulation against a plain fp64 loop (tests/timelimit_util.py), its bits
where no timeout occurs, the fixed point a truncated constant-reward episode must have, the storage's and the entry point's refusals,
the launcher's flag, and the kernel's resources in the built code object."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from solorl_amd import _native, build
from solorl_amd.ppo.storage import RolloutStorage
from tests import timelimit_util as tu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
T, N = 9, 5


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


@pytest.mark.parametrize("use_gae", [True, False])
def test_cpu_storage_path_matches_the_reference_loop(use_gae):
    """T = 9, N = 5 with a timeout at t = 0, one at t = T - 1, two on consecutive steps, a fall, and a flag where m == 1; the bound is
    the one the returns kernel is held to against its golden vectors (tests/test_parity_gpu.py: allclose, atol 1e-5)."""
    c = tu.make_case(T, N)
    m, f = c["masks"], c["timeouts"]
    assert (m[1, 0], f[0, 0], m[T, 1], f[T - 1, 1]) == (0, 1, 0, 1) and (m[4, 2], m[5, 2], f[3, 2], f[4, 2]) == (0, 0, 1, 1)
    assert (m[3, 3], f[2, 3], m[6, 4], f[5, 4]) == (0, 0, 1, 1)
    s = tu.storage_of(c, CPU)
    s.compute_returns(tu.next_value_of(c, CPU), use_gae, tu.GAMMA, tu.LAM)
    ref, vref = tu.reference_returns(c, use_gae)
    rows = slice(0, T) if use_gae else slice(0, T + 1)          # (GAE leaves returns[T] alone, as the reference's buffer does)
    err = float((s.returns[rows, :, 0].double() - torch.from_numpy(ref[rows])).abs().max())
    print("use_gae=%s: max |returns - fp64 loop| = %.3g" % (use_gae, err))
    assert torch.allclose(s.returns[rows, :, 0], torch.from_numpy(ref[rows]).float(), atol=1e-5)
    assert torch.equal(s.value_preds[:, :, 0], torch.from_numpy(vref).float())
    # and the flags matter: the loop that does not look at them gives other returns on the envs that were truncated
    plain, _ = tu.reference_returns(c, use_gae, bootstrap=False)
    assert np.abs(plain[0, 0] - ref[0, 0]) > 1e-2 and np.abs(plain[T - 1, 1] - ref[T - 1, 1]) > 1e-2
    assert np.array_equal(plain[:, 3], ref[:, 3])               # the fall


@pytest.mark.parametrize("use_gae", [True, False])
@pytest.mark.parametrize("flags", ["zero", "where_m_is_1"])
def test_cpu_returns_keep_their_bits_without_a_timeout(use_gae, flags):
    c = tu.make_case(T, N, seed=1)
    c["timeouts"] = np.zeros_like(c["timeouts"]) if flags == "zero" else (c["timeouts"] * (c["masks"][1:] == 1)).astype(np.uint8)
    assert flags == "zero" or c["timeouts"].sum() > 0
    a, b = tu.storage_of(c, CPU), tu.storage_of(c, CPU, bootstrap=False)
    assert b.timeouts is None
    for s in (a, b):
        s.compute_returns(tu.next_value_of(c, CPU), use_gae, tu.GAMMA, tu.LAM)
    assert torch.equal(a.returns, b.returns) and torch.equal(a.value_preds, b.value_preds)


@pytest.mark.parametrize("use_gae", [True, False])
def test_truncated_constant_reward_episodes_have_the_fixed_point(use_gae):
    """Reward 1 at every step, every episode cut off after L = 4 steps, T = 12, V = 1 / (1 - gamma) everywhere: with bootstrapping the
    returns are V and the advantages 0.  Bound: V = 100 lies in [64, 128), one float ulp there is 2^-17; delta_t = 1 + gamma V - V takes
    three roundings at that size (<= 2 ulp), an advantage sums at most L of them with weights < 1, and R = A + V rounds once more:
    10 ulp.  Without bootstrapping the returns saw-tooth: 1 at every last step, far below V everywhere."""
    L, T12, n = 4, 12, 3
    V = np.float32(1.0 / (1.0 - tu.GAMMA))
    c = dict(rewards=np.ones((T12, n), np.float32), values=np.full((T12 + 1, n), V, np.float32), masks=np.ones((T12 + 1, n), np.float32),
             timeouts=np.zeros((T12, n), np.uint8), next_value=np.full(n, V, np.float32))
    for t in range(L - 1, T12, L):
        c["masks"][t + 1], c["timeouts"][t] = 0, 1
    on, off = tu.storage_of(c, CPU), tu.storage_of(c, CPU, bootstrap=False)
    for s in (on, off):
        s.compute_returns(tu.next_value_of(c, CPU), use_gae, tu.GAMMA, tu.LAM)
    tol = 10 * 2.0 ** -17
    adv = on.returns[:-1] - on.value_preds[:-1]
    print("use_gae=%s: max |R - V| with bootstrapping %.3g (bound %.3g)" % (use_gae, float(adv.abs().max()), tol))
    assert float(adv.abs().max()) <= tol
    saw = off.returns[:-1, :, 0]
    assert torch.allclose(saw[L - 1::L], torch.ones(T12 // L, n), atol=1e-4)
    assert float((saw - float(V)).abs().min()) > 50.0
    assert bool((saw[:-1][torch.arange(T12 - 1) % L != L - 1] > saw[1:][torch.arange(T12 - 1) % L != L - 1]).all())     # falling inside an episode


def test_no_later_return_crosses_a_truncation_without_gae():
    """A truncated step takes V_t in the carry's place, as the kernel's select does -- not V_t plus 0 x the carry: a return that is not
    finite after the truncation leaves the returns before it finite.  (With GAE the advantage chain is cut by the factor m = 0 at
    every episode end, in the plain walk as here, so that mode is the plain one's and is not asked more.)"""
    c = tu.make_case(T, N, seed=4)
    c["masks"][:] = 1
    c["masks"][5], c["timeouts"][4] = 0, 1                     # every env truncated at t = 4
    c["rewards"][6] = np.inf
    s = tu.storage_of(c, CPU)
    s.compute_returns(tu.next_value_of(c, CPU), False, tu.GAMMA, tu.LAM)
    assert bool(torch.isfinite(s.returns[:5]).all()) and not bool(torch.isfinite(s.returns[5:7]).any())
    with np.errstate(invalid="ignore"):
        ref, _ = tu.reference_returns(c, False)
    assert torch.allclose(s.returns[:5, :, 0], torch.from_numpy(ref[:5]).float(), atol=1e-5)


def test_append_and_constructor_errors():
    row = lambda s, **kw: s.append(torch.zeros(N, 3), torch.zeros(N, 2), torch.zeros(N, 1), torch.zeros(N, 1), torch.zeros(N, 1), torch.ones(N, 1), **kw)
    plain, tl = RolloutStorage(T, N, (3,), 2, CPU), RolloutStorage(T, N, (3,), 2, CPU, bootstrap_timeouts=True)
    assert plain.timeouts is None and tl.timeouts.shape == (T, N, 1) and tl.timeouts.dtype == torch.uint8
    with pytest.raises(ValueError, match="timeouts goes with a storage made with bootstrap_timeouts"):
        row(plain, timeouts=torch.zeros(N, dtype=torch.uint8))
    with pytest.raises(ValueError, match="timeouts goes with a storage made with bootstrap_timeouts"):
        row(tl)
    assert plain.step == 0 and tl.step == 0                      # refused before anything was written
    flags = torch.tensor([0, 1, 0, 0, 1], dtype=torch.uint8)
    row(tl, timeouts=flags)                                      # [N], as the engine's info["timeout"]
    row(tl, timeouts=flags.unsqueeze(-1))
    assert torch.equal(tl.timeouts[0, :, 0], flags) and torch.equal(tl.timeouts[1, :, 0], flags) and tl.step == 2
    row(plain)
    assert plain.step == 1


def test_entry_point_refuses_bad_arguments_by_name(lib):
    """Decided before any HIP call: null arrays (the flags too -- no fallback to the plain returns), T < 1, N < 1"""
    p = C.c_void_p(4096)                                          # non-null, never dereferenced on the host
    good = [p] * 6 + [T, N, 1, 0.99, 0.95, 0, None]
    for k in range(6):
        args = list(good)
        args[k] = None
        assert lib.solorl_compute_returns_tl(*args) == -1, k
        assert lib.solorl_last_error().startswith(b"solorl_compute_returns_tl:") and b"null array" in lib.solorl_last_error(), k
    for t, n in ((0, N), (T, 0), (-3, N)):
        args = list(good)
        args[6], args[7] = t, n
        assert lib.solorl_compute_returns_tl(*args) == -1
        assert lib.solorl_last_error().startswith(b"solorl_compute_returns_tl:") and b"T and N" in lib.solorl_last_error()
    if not torch.cuda.is_available():
        assert lib.solorl_compute_returns_tl(*good) == -2 and b"no CPU fallback" in lib.solorl_last_error()


def test_binding_and_header_declare_the_entry_point(lib):
    hdr = open(os.path.join(ROOT, "include", "solorl.h")).read()
    assert re.search(r"^int solorl_compute_returns_tl\(", hdr, re.M) and re.search(r"^ \*   solorl_compute_returns_tl\s+:", hdr, re.M)
    assert "solorl_compute_returns_tl" in _native.SYMBOLS
    f = lib.solorl_compute_returns_tl
    assert f.restype is C.c_int and len(f.argtypes) == len(lib.solorl_compute_returns.argtypes) + 1 == 13
    assert re.search(r"#define SOLORL_ABI_VERSION 5\b", hdr)      # no struct changed its layout


def test_kernel_keeps_the_plain_kernels_occupancy_without_scratch(lib):
    """The flag row costs a few registers and nothing else: no scratch, no LDS, no spills, and at most 72 VGPRs -- the most at which
    seven wavefronts fit a SIMD (512 / 7, in allocation units of 8), which is what the plain returns kernel reaches."""
    from solorl_amd import devcode
    res = devcode.kernel_resources(build.LIB)
    tl = [v for k, v in res.items() if "returns_tl_kernel" in k]
    plain = [v for k, v in res.items() if "returns_kernel" in k]
    assert tl and plain
    for v in tl:
        print("returns_tl_kernel:", v["vgpr_count"], "VGPRs,", v["sgpr_count"], "SGPRs (plain: %d VGPRs)" % plain[0]["vgpr_count"])
        assert v["private_segment_fixed_size"] == 0 and v["group_segment_fixed_size"] == 0
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["agpr_count"] == 0
        assert v["vgpr_count"] <= 72


def test_launcher_flag():
    """train_ppo.py --bootstrap-timeouts parses, and the reference's README command line leaves it off"""
    sys.path.insert(0, ROOT)
    import train_ppo
    assert train_ppo.get_ppo_args(["--bootstrap-timeouts"]).bootstrap_timeouts is True
    a = train_ppo.get_ppo_args("--num-agents 64 --logdir /tmp/L --log-interval 5 --save-interval 50 --lr 0.00025 --entropy-coef 0.01 "
                               "--clip-param 0.1 --ppo-epoch 5 --mini-batch-size 512 --clip-value-loss --config-file ./configs/basic.yaml "
                               "--use-gae --use-linear-lr-decay --seed 1".split())
    assert a.bootstrap_timeouts is False and a.use_gae and a.num_agents == 64
