"""Running normalisation (include/solorl.h solorl_normalize_obs / solorl_normalize_rewards, solorl_amd/normalize.py) without a GPU: the
fp64 restatement the GPU tests use reproduces the reference's recorded VecNormalize run within the recorded float32-vs-float64 gap, the
entry points follow the error convention before any HIP call, the kernels use no scratch registers, and the defaults change nothing."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from solorl_amd import _native, build
from tests import norm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "norm_golden.npz")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _native.lib()


@pytest.mark.parametrize("n", [5, 67])
def test_restatement_reproduces_the_reference(n):
    """The yardstick itself: tests/norm_ref.py, run over the recorded raw inputs, gives the reference's outputs within the recorded
    differences (which the generator measured with this same code: equality up to nothing), its float32 observation statistics within
    float32 rounding of the fp64 ones, and its float64 return statistics and accumulators to fp64 rounding."""
    g = np.load(GOLDEN)
    k = lambda name: g["%s_n%d" % (name, n)]
    obs, rew, done = k("obs_raw"), k("rew_raw"), k("done")
    T, D = rew.shape[0], obs.shape[2]
    assert obs.shape == (T + 1, n, D) and D == 42 and T >= 24 and 0.1 < done.mean() < 0.3
    assert (np.abs(k("obs_ref")) == 10.0).sum() >= 3 and (np.abs(k("rew_ref")) == 10.0).sum() >= 1       # some entries clipped
    R = norm_ref.NormRef(n, D)
    o = [R.obs(obs[0])]
    R.reset()
    dmean = dvar = 0.0
    for t in range(T):
        r = R.rewards(rew[t], done[t])
        o.append(R.obs(obs[t + 1]))
        assert np.abs(r - k("rew_ref")[t]).max() <= k("ref_vs_f64_rew")
        # float64 on both sides: summation order only
        assert abs(R.rt.mean - k("rt_mean")[t]) <= 1e-12 * np.abs(k("ret")).max() and abs(R.rt.var - k("rt_var")[t]) <= 1e-12 * (k("ret") ** 2).max()
        assert R.rt.count == k("rt_count")[t]
        assert np.abs(R.ret - k("ret")[t]).max() <= 1e-12 * np.abs(k("ret")).max()
        assert (R.ret[done[t]] == 0).all()
        dmean = max(dmean, (np.abs(R.ob.mean - k("ob_mean")[t + 1]) / np.abs(obs).max(axis=(0, 1))).max())
        dvar = max(dvar, (np.abs(R.ob.var - k("ob_var")[t + 1]) / (obs.astype(np.float64) ** 2).max(axis=(0, 1))).max())
    assert np.abs(np.stack(o) - k("obs_ref")).max() <= k("ref_vs_f64_obs")
    assert k("ref_vs_f64_obs") < 1e-3 and k("ref_vs_f64_rew") < 1e-9          # the gap is float32 statistics, not another formula
    # the reference's float32 statistics: a few float32 roundings per step of quantities bounded by the column's largest |x| / x^2
    assert dmean < 64 * 2.0 ** -24 and dvar < 64 * 2.0 ** -24, (dmean, dvar)


def test_symbols_and_error_convention(lib):
    for s in ("solorl_norm_scratch_count", "solorl_normalize_obs", "solorl_normalize_rewards"):
        assert s in _native.SYMBOLS and hasattr(lib, s)
    p = 4096           # non-null, never dereferenced: every check below fails before any HIP call
    ok_obs = dict(stats=p, rows=2, n=8, D=42, obs_in=p, obs_out=p, update=1, clip=10.0, eps=1e-8, scratch=p, dev=0, stream=None)
    for bad in (dict(stats=None), dict(obs_in=None), dict(obs_out=None), dict(scratch=None), dict(rows=0), dict(n=0), dict(D=0), dict(n=-3)):
        a = dict(ok_obs, **bad)
        assert lib.solorl_normalize_obs(*a.values()) == -1, bad
        assert b"solorl_normalize_obs" in lib.solorl_last_error(), bad
    ok_rew = dict(stats=p, ret=p, rows=2, n=8, rewards=p, done=p, update=1, gamma=0.99, clip=10.0, eps=1e-8, scratch=p, dev=0, stream=None)
    for bad in (dict(stats=None), dict(ret=None), dict(rewards=None), dict(done=None), dict(scratch=None), dict(rows=0), dict(n=0)):
        a = dict(ok_rew, **bad)
        assert lib.solorl_normalize_rewards(*a.values()) == -1, bad
        assert b"solorl_normalize_rewards" in lib.solorl_last_error(), bad
    for rows, n, D in ((0, 8, 42), (1, 0, 42), (1, 8, 0), (-1, -1, -1)):
        assert lib.solorl_norm_scratch_count(rows, n, D) == 0
    # a count that grows with every argument and covers at least the per-row statistics (and, for the returns, the [rows][n] accumulators)
    c = lib.solorl_norm_scratch_count
    assert c(1, 67, 42) >= 2 * 42 + 1 and c(2, 67, 42) > c(1, 67, 42) and c(1, 4099, 42) > c(1, 67, 42) and c(1, 67, 84) > c(1, 67, 42)
    assert c(37, 67, 1) >= 37 * 67
    import torch
    if not torch.cuda.is_available():                 # valid arguments: no silent fallback without a GPU
        assert lib.solorl_normalize_obs(*ok_obs.values()) == -2 and b"no CPU fallback" in lib.solorl_last_error()
        assert lib.solorl_normalize_rewards(*ok_rew.values()) == -2 and b"no CPU fallback" in lib.solorl_last_error()


def test_running_mean_std_round_trip(tmp_path):
    import torch
    from solorl_amd.normalize import RunningMeanStd
    r = RunningMeanStd(shape=(42,))
    assert r.mean.shape == (42,) and (r.mean == 0).all() and (r.var == 1).all() and r.count == 1e-4        # running_mean_std.py:13-16
    rng = np.random.default_rng(0)
    x = rng.standard_normal((9, 42)) * 3 + 1
    r.update(x)
    ref = norm_ref.Stats((42,))
    ref.update(x)
    assert np.array_equal(r.mean, ref.mean) and np.array_equal(r.var, ref.var) and r.count == ref.count
    path = str(tmp_path / "ck.pt")
    torch.save({"ob_rms": r, "ret_rms": RunningMeanStd(shape=())}, path)
    back = torch.load(path, map_location="cpu", weights_only=False)
    assert isinstance(back["ob_rms"], RunningMeanStd) and back["ret_rms"].mean.shape == ()
    assert np.array_equal(back["ob_rms"].mean, r.mean) and np.array_equal(back["ob_rms"].var, r.var) and back["ob_rms"].count == r.count
    # the device layout, on the host: mean[D], var[D], count in fp64 -- and back
    t = r.to_device("cpu")
    assert t.dtype == torch.float64 and np.array_equal(t.numpy(), ref.flat())
    q = RunningMeanStd(shape=(42,)).from_device(t)
    assert np.array_equal(q.mean, r.mean) and np.array_equal(q.var, r.var) and q.count == r.count
    s = RunningMeanStd(shape=()).from_device(RunningMeanStd(shape=()).to_device("cpu"))
    assert s.mean.shape == () and s.var == 1.0 and s.count == 1e-4


def test_norm_kernels_use_no_scratch(lib):
    from solorl_amd import devcode
    res = {k: v for k, v in devcode.kernel_resources(build.LIB).items() if "norm_" in k}
    assert len(res) >= 6, sorted(res)
    for k, v in res.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert not any(p in k for p in ("step_kernel", "rollout_kernel", "phase_", "pgs_team")), k       # (patterns other static tests select by)


def test_defaults_change_nothing():
    from solorl_amd import vec_env
    sig = inspect.signature(vec_env.make_vec_envs).parameters
    assert (sig["norm_obs"].default, sig["norm_ret"].default, sig["clipob"].default, sig["cliprew"].default, sig["epsilon"].default) == (False, False, 10.0, 10.0, 1e-8)
    # without a device the constructor fails before anything else; the attributes are checked on a bare instance
    e = vec_env.SoloVecEnv.__new__(vec_env.SoloVecEnv)
    e._norm, e._norm_obs, e._norm_ret, e.closed = None, False, False, True
    assert e.ob_rms is None and e.ret_rms is None
    e.ob_rms = None                     # (what loading a checkpoint without statistics does)
    with pytest.raises(_native.SoloRLError):
        e.ob_rms = object()
    e.training = True
    e.eval()
    assert e.training is False
    e.train()
    assert e.training is True
