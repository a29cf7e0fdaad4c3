"""Running normalisation on the GPU (include/solorl.h solorl_normalize_obs / solorl_normalize_rewards; SoloVecEnv norm_obs / norm_ret)
against the fp64 restatement of the reference's formulas (tests/norm_ref.py) and the reference's recorded VecNormalize run
(tests/golden/norm_golden.npz), plus determinism, graph capture and the path through the env.

Bounds.  Statistics: |d mean| <= 1e-12 max|x|, |d var| <= 1e-12 max x^2 -- fp64 sums of at most 4099 terms in another order
(4099 x 2^-53 = 4.6e-13 relative to the largest term, worst case).  Outputs: within 1 float32 ulp of the restatement's value rounded
to float32 (both round one fp64 value whose inputs differ by ~1e-12).  Against the reference: its recorded distance to the
restatement + 2e-6 for observations (1 ulp of a value <= 10 is 9.5e-7), + 1 ulp of the reward for rewards."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import norm_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "norm_golden.npz")
DEV = "cuda:0"
NS = (1, 5, 64, 67, 4099)
ROWS = 12


def _lib():
    from solorl_amd import _native
    return _native


def _fresh_stats(D):
    from solorl_amd.normalize import RunningMeanStd
    return RunningMeanStd(shape=(D,) if D > 1 else ()).to_device(torch.device(DEV))


def _scratch(rows, n, D):
    k = _lib().lib().solorl_norm_scratch_count(rows, n, D)
    assert k > 0
    return torch.full((k,), float("nan"), dtype=torch.float64, device=DEV)           # (nothing may be read before it is written)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def norm_obs(stats, x, out, update, clip=10.0, eps=1e-8, scratch=None):
    rows, n, D = x.shape
    s = _scratch(rows, n, D) if scratch is None else scratch
    N = _lib()
    N.check(N.lib().solorl_normalize_obs(stats.data_ptr(), rows, n, D, x.data_ptr(), out.data_ptr(), update, clip, eps, s.data_ptr(), 0, _stream()))
    return out


def norm_rew(stats, ret, r, done, update, gamma=0.99, clip=10.0, eps=1e-8, scratch=None):
    rows, n = r.shape
    s = _scratch(rows, n, 1) if scratch is None else scratch
    N = _lib()
    N.check(N.lib().solorl_normalize_rewards(stats.data_ptr(), ret.data_ptr(), rows, n, r.data_ptr(), done.data_ptr(), update, gamma, clip, eps,
                                             s.data_ptr(), 0, _stream()))
    return r


def _obs_inputs(n, D, rows=ROWS, seed=0):
    rng = np.random.default_rng(1000 * n + D + seed)
    scale = np.geomspace(1e-2, 30.0, D)
    mean = rng.uniform(-3.0, 3.0, D) * scale
    x = (mean + scale * rng.standard_normal((rows, n, D))).astype(np.float32)
    if n >= 64:                     # far outliers in the last row: |normalised| <= sqrt(count), so only there can they pass the clip of 10
        for _ in range(5):
            e, d = rng.integers(n), rng.integers(D)
            x[rows - 1, e, d] = np.float32(mean[d] + scale[d] * rng.choice([-1000.0, 1000.0]))
    return x


_OBS_REF = {}


def _obs_ref(n, D):
    """restatement over the 12 rows, computed once per shape and shared: (inputs, fp64 outputs [rows][n][D], final stats)"""
    if (n, D) not in _OBS_REF:
        x = _obs_inputs(n, D)
        R = norm_ref.NormRef(n, D)
        y = np.stack([R.obs(x[t]) for t in range(x.shape[0])])
        _OBS_REF[(n, D)] = (x, y, R.ob.flat())
    return _OBS_REF[(n, D)]


def _check_stats(got, want, D, xmax, what):
    got = got.cpu().numpy()
    dm, dv = np.abs(got[:D] - want[:D]).max(), np.abs(got[D:2 * D] - want[D:2 * D]).max()
    print("%s: |d mean| %.3e (bound %.3e)  |d var| %.3e (bound %.3e)" % (what, dm, 1e-12 * xmax, dv, 1e-12 * xmax ** 2))
    assert dm <= 1e-12 * xmax and dv <= 1e-12 * xmax ** 2, what
    assert got[2 * D] == want[2 * D], what                      # count: the same additions


def _check_out(got, want64, what):
    want = want64.astype(np.float32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst = (err / norm_ref.ulp32(want)).max()
    print("%s: worst output error %.3f ulp" % (what, worst))
    assert worst <= 1.0, what


@pytest.mark.parametrize("D", [30, 42, 84])
@pytest.mark.parametrize("n", NS)
def test_obs_against_the_restatement(gpu_device, n, D):
    x, y, stats_ref = _obs_ref(n, D)
    xd = torch.from_numpy(x).to(DEV)
    stats, out = _fresh_stats(D), torch.empty_like(xd)
    norm_obs(stats, xd, out, 1)                                  # one call over the 12 rows, out of place
    torch.cuda.synchronize()
    _check_stats(stats, stats_ref, D, float(np.abs(x).max()), "obs n=%d D=%d" % (n, D))
    got = out.cpu().numpy()
    _check_out(got, y, "obs n=%d D=%d" % (n, D))
    clipped = np.abs(y) == 10.0
    assert (np.abs(got[clipped]) == 10.0).all() and (np.sign(got[clipped]) == np.sign(y[clipped])).all()     # exactly +-clip
    assert np.abs(got).max() <= 10.0
    if n >= 64:
        assert clipped.sum() >= 1
    if n == 1:                                                   # a batch of one: variance exactly 0 merged in; finite everywhere
        assert np.isfinite(got).all()
    # in place, row by row: bitwise the out-of-place rows and statistics
    s2, x2 = _fresh_stats(D), xd.clone()
    for t in range(ROWS):
        norm_obs(s2, x2[t:t + 1], x2[t:t + 1], 1)
    assert torch.equal(x2, out) and torch.equal(s2, stats)
    # update = 0: the statistics stay bitwise, the output is the scaling by them
    s3 = stats.clone()
    o3 = norm_obs(s3, xd[:2], torch.empty_like(xd[:2]), 0)
    assert torch.equal(s3, stats)
    sr = stats_ref
    want = np.clip((x[:2].astype(np.float64) - sr[:D]) / np.sqrt(sr[D:2 * D] + 1e-8), -10.0, 10.0)
    _check_out(o3.cpu().numpy(), want, "obs update=0 n=%d D=%d" % (n, D))


def _rew_inputs(n, rows, seed=0):
    rng = np.random.default_rng(77 * n + rows + seed)
    r = (0.3 + 0.5 * rng.standard_normal((rows, n))).astype(np.float32)
    if rows > 1 and n >= 5:
        r[rows - 1, rng.integers(n)] = np.float32(-1000.0)        # beyond the clip
    done = (rng.random((rows, n)) < 0.2).astype(np.uint8)
    return r, done


@pytest.mark.parametrize("rows", [1, 37])
@pytest.mark.parametrize("n", NS)
def test_rewards_against_the_restatement(gpu_device, n, rows):
    r, done = _rew_inputs(n, rows)
    R = norm_ref.NormRef(n, 1)
    R.ret = np.random.default_rng(n).standard_normal(n) * 2.0     # accumulators in mid-episode
    ret0 = R.ret.copy()
    want, pre = [], []              # pre: the accumulators before their row's zeroing -- the x the statistics are taken of
    for t in range(rows):
        pre.append(R.ret * 0.99 + r[t].astype(np.float64))
        want.append(R.rewards(r[t], done[t]))
    acc_hi = float(np.abs(np.stack(pre)).max())
    # one call over all rows
    stats, ret = _fresh_stats(1), torch.from_numpy(ret0).to(DEV)
    rd, dd = torch.from_numpy(r).to(DEV), torch.from_numpy(done).to(DEV)
    one = norm_rew(stats, ret, rd.clone(), dd, 1)
    torch.cuda.synchronize()
    what = "rew n=%d rows=%d" % (n, rows)
    _check_stats(stats, R.rt.flat(), 1, acc_hi, what)
    dret = np.abs(ret.cpu().numpy() - R.ret).max()
    print("%s: |d ret| %.3e (bound %.3e)" % (what, dret, 1e-12 * acc_hi))
    assert dret <= 1e-12 * acc_hi
    _check_out(one.cpu().numpy(), np.stack(want), what)
    if rows > 1 and n >= 5:
        assert (one.cpu().numpy() == -10.0).sum() >= 1
    # row by row: bitwise the same rewards, statistics and accumulators; a done env enters the next row with ret = 0
    s2, ret2, r2 = _fresh_stats(1), torch.from_numpy(ret0).to(DEV), rd.clone()
    for t in range(rows):
        norm_rew(s2, ret2, r2[t:t + 1], dd[t:t + 1], 1)
        assert (ret2[dd[t].bool()] == 0).all() and (ret2[~dd[t].bool()] != 0).all()
    assert torch.equal(r2, one) and torch.equal(s2, stats) and torch.equal(ret2, ret)
    # update = 0: statistics bitwise untouched, accumulators still advance, rewards scaled by the frozen variance
    s3, ret3 = stats.clone(), torch.from_numpy(ret0).to(DEV)
    o3 = norm_rew(s3, ret3, rd.clone(), dd, 0)
    assert torch.equal(s3, stats) and torch.equal(ret3, ret)
    _check_out(o3.cpu().numpy(), np.clip(r.astype(np.float64) / np.sqrt(R.rt.var + 1e-8), -10.0, 10.0), what + " update=0")


@pytest.mark.parametrize("n", [5, 67])
def test_against_the_reference_golden(gpu_device, n):
    g = np.load(GOLDEN)
    k = lambda name: g["%s_n%d" % (name, n)]
    obs, rew, done = k("obs_raw"), k("rew_raw"), k("done").astype(np.uint8)
    D = obs.shape[2]
    stats = _fresh_stats(D)
    out = norm_obs(stats, torch.from_numpy(obs).to(DEV), torch.empty(obs.shape, device=DEV), 1).cpu().numpy()       # reset's row, then every step's
    err = np.abs(out.astype(np.float64) - k("obs_ref").astype(np.float64)).max()
    print("golden n=%d: obs |engine - reference| %.3e (recorded reference-vs-fp64 %.3e)" % (n, err, k("ref_vs_f64_obs")))
    assert err <= k("ref_vs_f64_obs") + 2e-6
    rs, ret = _fresh_stats(1), torch.zeros(n, dtype=torch.float64, device=DEV)
    r = norm_rew(rs, ret, torch.from_numpy(rew).to(DEV), torch.from_numpy(done).to(DEV), 1).cpu().numpy()
    err = np.abs(r.astype(np.float64) - k("rew_ref"))
    print("golden n=%d: rew |engine - reference| max %.3e (recorded %.3e)" % (n, err.max(), k("ref_vs_f64_rew")))
    assert (err <= k("ref_vs_f64_rew") + norm_ref.ulp32(k("rew_ref"))).all()
    # and its statistics / accumulators after the last step: float64 in the reference, the statistics bounds above
    pre = np.concatenate([np.zeros((1, n)), k("ret")[:-1]]) * 0.99 + rew.astype(np.float64)       # the accumulators before their row's zeroing
    _check_stats(rs, np.array([k("rt_mean")[-1], k("rt_var")[-1], k("rt_count")[-1]]), 1, float(np.abs(pre).max()), "golden ret n=%d" % n)
    assert np.abs(ret.cpu().numpy() - k("ret")[-1]).max() <= 1e-12 * np.abs(pre).max()


def _sequence(n, D, steps, seed):
    return [(torch.from_numpy(_obs_inputs(n, D, rows=1, seed=seed + i)).to(DEV),) + tuple(torch.from_numpy(a).to(DEV) for a in _rew_inputs(n, 1, seed=seed + i))
            for i in range(steps)]


def test_deterministic_and_capturable(gpu_device):
    n, D, steps = 4099, 42, 3
    seq = _sequence(n, D, steps, 5)
    so, sr = _scratch(1, n, D), _scratch(1, n, 1)

    def eager():
        st, rs, ret = _fresh_stats(D), _fresh_stats(1), torch.zeros(n, dtype=torch.float64, device=DEV)
        outs = []
        for x, r, d in seq:
            o = norm_obs(st, x, torch.empty_like(x), 1, scratch=so)
            rr = norm_rew(rs, ret, r.clone(), d, 1, scratch=sr)
            outs.append((o, rr))
        return st, rs, ret, outs
    a, b = eager(), eager()
    for i in range(3):
        assert torch.equal(a[i], b[i])
    for (o1, r1), (o2, r2) in zip(a[3], b[3]):
        assert torch.equal(o1, o2) and torch.equal(r1, r2)
    # the same pair of calls captured once as a linear chain, replayed on fresh inputs
    st, rs, ret = _fresh_stats(D), _fresh_stats(1), torch.zeros(n, dtype=torch.float64, device=DEV)
    x, r, d = (torch.empty_like(t) for t in seq[0])
    o = torch.empty_like(x)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        norm_obs(st, x, o, 1, scratch=so)
        norm_rew(rs, ret, r, d, 1, scratch=sr)
    for i, (xi, ri, di) in enumerate(seq):
        x.copy_(xi); r.copy_(ri); d.copy_(di)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o, a[3][i][0]) and torch.equal(r, a[3][i][1]), i
    assert torch.equal(st, a[0]) and torch.equal(rs, a[1]) and torch.equal(ret, a[2])


# ---------------------------------------------------------------------------------------------------------------- through the env
N_ENV = 67


def _cfg():
    from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
    c = default_config(ROBOT_SOLO12, TASK_WALK); c.num_history_stack = 1; c.episode_length = 25
    return c


def _policy(O=76, A=12, seed=3):
    from solorl_amd.ppo import Policy
    from solorl_amd.vec_env import Box
    torch.manual_seed(seed)
    pol = Policy((O,), Box(-np.ones(A), np.ones(A)), None, {"hidden_size": 64}).to(DEV)
    with torch.no_grad():
        pol.pi_dist.logstd.normal_(0, 0.3)
    return pol


def test_defaults_give_no_normaliser(gpu_device):
    from solorl_amd.vec_env import make_vec_envs
    env = make_vec_envs(_cfg(), 8, device=torch.device(DEV))
    assert env.ob_rms is None and env.ret_rms is None and env._norm is None and env.training is True
    env.close()


def test_norm_obs_through_the_env(gpu_device):
    """reset / step_inplace into a storage row / step / step_n on an env with norm_obs, against a raw twin env whose rows go through a
    twin normaliser: bitwise.  get_observation stays raw; eval() freezes the statistics; reset_masked normalises the selected rows only."""
    from solorl_amd.normalize import VecNormalizer
    from solorl_amd.vec_env import make_vec_envs, SoloVecEnv
    dev = torch.device(DEV)
    env = make_vec_envs(_cfg(), N_ENV, device=dev, seed=5, norm_obs=True)
    raw = SoloVecEnv(_cfg(), N_ENV, device=dev, seed=5)
    twin = VecNormalizer(N_ENV, 76, dev, True, False)
    assert env.ret_rms is None and env.ob_rms.mean.shape == (76,) and env.ob_rms.count == 1e-4
    o = env.reset()
    assert torch.equal(o, twin.obs(raw.reset(), 1, True))
    assert torch.equal(env.get_observation(), raw.get_observation())
    g = torch.Generator(device=DEV); g.manual_seed(3)
    row, rrow = torch.empty(N_ENV, 76, device=dev), torch.empty(N_ENV, 1, device=dev)
    for t in range(4):
        a = torch.rand(N_ENV, 12, device=dev, generator=g) * 2 - 1
        o, r, d, _ = env.step_inplace(a, obs_out=row, rew_out=rrow)
        o2, r2, d2, _ = raw.step_inplace(a)
        assert o is row and torch.equal(row, twin.obs(o2.clone(), 1, True)) and torch.equal(rrow.view(-1), r2) and torch.equal(d, d2)
    assert torch.equal(env._norm.ob_stats, twin.ob_stats)
    a = torch.rand(N_ENV, 12, device=dev, generator=g) * 2 - 1
    o, r, dn, _ = env.step(a)
    o2, r2, _, _ = raw.step(a)
    assert torch.equal(o, twin.obs(o2, 1, True)) and torch.equal(r, r2)
    acts = torch.rand(3, N_ENV, 12, device=dev, generator=g) * 2 - 1
    o, _, _, _ = env.step_n_inplace(acts)
    o2, _, _, _ = raw.step_n_inplace(acts)
    assert torch.equal(o, twin.obs(o2.clone(), 3, True)) and torch.equal(env._norm.ob_stats, twin.ob_stats)
    rms = env.ob_rms
    assert np.array_equal(rms.mean, twin.ob_stats[:76].cpu().numpy()) and abs(rms.count - (1e-4 + 9 * N_ENV)) < 1e-9
    # eval(): the statistics freeze, the scaling goes on
    env.eval()
    before = env._norm.ob_stats.clone()
    o, _, _, _ = env.step_inplace(a)
    o2, _, _, _ = raw.step_inplace(a)
    assert torch.equal(env._norm.ob_stats, before) and torch.equal(o, twin.obs(o2.clone(), 1, False))
    mask = torch.zeros(N_ENV, dtype=torch.bool, device=dev); mask[::3] = True
    o, o2 = env.reset_masked(mask), raw.reset_masked(mask)
    assert torch.equal(env._norm.ob_stats, before)
    assert torch.equal(o[mask], twin.obs(o2.clone(), 1, False)[mask]) and torch.equal(o[~mask], o2[~mask])
    env.train()
    env.step_inplace(a)
    assert not torch.equal(env._norm.ob_stats, before)
    # assigning statistics uploads them (what loading a checkpoint does)
    env.ob_rms = rms
    assert torch.equal(env._norm.ob_stats, rms.to_device(dev))
    env.close(); raw.close()


def test_graphed_rollout_with_norm_obs(gpu_device):
    from solorl_amd.normalize import VecNormalizer
    from solorl_amd.ppo import RolloutStorage
    from solorl_amd.ppo.fused import policy_params
    from solorl_amd.ppo.graphs import GraphedRollout
    from solorl_amd.vec_env import make_vec_envs, SoloVecEnv
    dev, T = torch.device(DEV), 6
    pol = _policy()
    env = make_vec_envs(_cfg(), N_ENV, device=dev, seed=9, norm_obs=True)
    assert not env.step_act_supported(policy_params(pol)) and not env.rollout_supported(policy_params(pol))
    with pytest.raises(_lib().SoloRLError):
        env.rollout_inplace(torch.zeros(2, N_ENV, 12, device=dev), policy_params(pol), None, torch.zeros(2, N_ENV, device=dev), torch.zeros(2, N_ENV, device=dev))
    st = RolloutStorage(T, N_ENV, (76,), 12, dev)
    st.obs[0].copy_(env.reset())
    with torch.no_grad():
        pol.act(st.obs[0])
    roll = GraphedRollout(env, pol, st, T)
    roll()
    torch.cuda.synchronize()
    assert roll.graph is not None and not roll.step_act
    # the stored actions replayed on a raw twin env + twin normaliser reproduce every stored (normalised) row
    raw, twin = SoloVecEnv(_cfg(), N_ENV, device=dev, seed=9), VecNormalizer(N_ENV, 76, dev, True, False)
    assert torch.equal(st.obs[0], twin.obs(raw.reset(), 1, True))
    for t in range(T):
        o, r, d, _ = raw.step_inplace(st.actions[t].contiguous())
        assert torch.equal(st.obs[t + 1], twin.obs(o.clone(), 1, True)), t
        assert torch.equal(st.rewards[t].view(-1), r) and torch.equal(st.masks[t + 1].view(-1), 1.0 - d.float())
    assert torch.equal(env._norm.ob_stats, twin.ob_stats)
    with torch.no_grad():                                   # the policy acted on the normalised rows
        v, lp, _ = pol.evaluate_actions(st.obs[T - 1], st.actions[T - 1])
    assert torch.allclose(v, st.value_preds[T - 1], atol=1e-5)
    env.close(); raw.close()


def test_norm_ret_rollout_equals_step_act_calls(gpu_device):
    """norm_ret alone keeps the fused paths: rollout_inplace with K = 4 (one reward call over the window's 4 rows, after it) against four
    step_act_inplace calls (one reward call each), bitwise in rewards, statistics and accumulators -- and the raw rewards of a twin env
    through the restatement, within 1 ulp."""
    from solorl_amd.ppo.fused import policy_params
    from solorl_amd.vec_env import make_vec_envs, SoloVecEnv
    dev, K = torch.device(DEV), 4
    P = policy_params(_policy())
    e1 = make_vec_envs(_cfg(), N_ENV, device=dev, seed=5, norm_ret=True, gamma=0.97)
    e2 = make_vec_envs(_cfg(), N_ENV, device=dev, seed=5, norm_ret=True, gamma=0.97)
    raw = SoloVecEnv(_cfg(), N_ENV, device=dev, seed=5)
    assert e1.ob_rms is None and e1.step_act_supported(P) and e1.rollout_supported(P)
    o1 = e1.reset()
    assert torch.equal(o1, e2.reset()) and torch.equal(o1, raw.reset())
    g = torch.Generator(device=DEV); g.manual_seed(13)
    a0 = torch.rand(N_ENV, 12, device=dev, generator=g) * 2 - 1
    Rf, ended = norm_ref.NormRef(N_ENV, 1, gamma=0.97), 0
    for w in range(8):                                     # 32 steps: episodes (25 steps) end inside
        noise = torch.randn(K + 1, N_ENV, 12, device=dev, generator=g)
        act = torch.zeros(K + 1, N_ENV, 12, device=dev); act[0] = a0
        val, lp = torch.zeros(K + 1, N_ENV, device=dev), torch.zeros(K + 1, N_ENV, device=dev)
        rews, dones = [], []
        for k in range(K):
            o, r, d, _ = e1.step_act_inplace(act[k], P, noise[k + 1].contiguous(), val[k + 1], act[k + 1], lp[k + 1])
            rews.append(r.clone()); dones.append(d.clone())
        act2 = torch.zeros_like(act); act2[0] = a0
        o2, r2, d2, _ = e2.rollout_inplace(act2, P, noise, torch.zeros_like(val), torch.zeros_like(lp), policy_after_last=True)
        assert torch.equal(act, act2) and torch.equal(torch.stack(rews), r2) and torch.equal(torch.stack(dones), d2), w
        assert torch.equal(e1._norm.ret_stats, e2._norm.ret_stats) and torch.equal(e1._norm.ret, e2._norm.ret), w
        rr = torch.stack([raw.step_inplace(act[k].contiguous())[1].clone() for k in range(K)]).cpu().numpy()
        dn = d2.cpu().numpy()
        _check_out(r2.cpu().numpy(), np.stack([Rf.rewards(rr[k], dn[k]) for k in range(K)]), "env rewards window %d" % w)
        assert not np.array_equal(rr, r2.cpu().numpy())
        ended += int(dn.sum())
        a0 = act[K].clone()
    rms = e1.ret_rms
    assert rms.mean.shape == () and abs(rms.count - (1e-4 + 32 * N_ENV)) < 1e-9 and rms.var > 0
    assert ended > 0
    for e in (e1, e2, raw):
        e.close()


def test_checkpoint_carries_the_statistics_and_eval_loads_it(gpu_device, tmp_path, monkeypatch):
    import sys
    import types
    from solorl_amd import vec_env
    from solorl_amd.config import load_yaml
    from solorl_amd.normalize import RunningMeanStd
    from solorl_amd.ppo.train import train
    config = load_yaml(os.path.join(ROOT, "configs", "basic12.yaml"))
    config["task"] = "walk"
    made = []
    real = vec_env.make_vec_envs
    monkeypatch.setattr(vec_env, "make_vec_envs", lambda *a, **k: made.append(real(*a, **k)) or made[-1])
    args = types.SimpleNamespace(
        num_agents=64, hidden_size=64, cuda=True, gamma=0.99, tau=0.95, clip_param=0.1, ppo_epoch=1, mini_batch_size=512,
        lr=2.5e-4, l2_coef=0.0, value_loss_coef=0.5, entropy_coef=0.01, max_grad_norm=0.5, use_linear_lr_decay=False,
        use_gae=True, num_env_steps=64 * 16 * 2, seed=1, curriculum_schedule=0, log_interval=1, logdir=str(tmp_path),
        base_checkpoint=None, save_interval=1, num_steps=16, normalize_obs=True, normalize_returns=True)
    pol, hist = train(args, config)
    assert len(hist) == 2 and all(torch.isfinite(p).all() for p in pol.parameters())
    env = made[0]
    ck = torch.load(os.path.join(str(tmp_path), "solo.pt"), weights_only=False)
    assert set(ck.keys()) == {"update", "state_dict", "ob_rms", "ret_rms"}
    assert isinstance(ck["ob_rms"], RunningMeanStd) and isinstance(ck["ret_rms"], RunningMeanStd)
    D = env.obs_dim
    assert np.array_equal(ck["ob_rms"].mean, env._norm.ob_stats[:D].cpu().numpy()) and np.array_equal(ck["ob_rms"].var, env._norm.ob_stats[D:2 * D].cpu().numpy())
    assert abs(ck["ob_rms"].count - (1e-4 + 64 * (1 + 2 * 16))) < 1e-9 and abs(ck["ret_rms"].count - (1e-4 + 64 * 2 * 16)) < 1e-9
    sys.path.insert(0, ROOT)
    import eval_ppo
    r = eval_ppo.main(["--checkpoint-dir", str(tmp_path), "--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk",
                       "--num-runs", "4", "--num-agents", "16"])
    assert r["episodes"] >= 4 and 1 <= r["mean_length"] <= 400
    assert made[1].training is False and np.array_equal(made[1].ob_rms.mean, ck["ob_rms"].mean)
