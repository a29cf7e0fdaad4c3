"""Observation noise and actuation on the GPU (include/solorl.h solorl_obs_noise / solorl_actuate; solorl_amd/channel.py and
SoloVecEnv.set_obs_noise / set_actuation).  Both kernels against the host program (csrc/channel.hpp compiled alone by g++) and the Python
prediction of tests/channel_util.py, bitwise; then twin handles: noise changes the observations and nothing else, actuation is exactly
"the twin stepped with the predicted applied actions"; capture, the policy tail, the refusals, PPO with the three flags and eval_ppo.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from solorl_amd import _native, channel
from solorl_amd.config import default_config, ROBOT_SOLO12, TASK_WALK
from tests import channel_util as cu
from tests.host_util import build_host
from tests.test_channel_host import ACT_CASES, RESTARTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SIZES = (1, 5, 65, 257)            # one row, a partial workgroup, several workgroups with a partial last one
SEED, OFF = 2301, 2 ** 32 + 3      # (global env ids above 2^32)


@pytest.fixture(scope="module")
def exe():
    return build_host("channel_main")


def _rows(n, D, offset_words, seed):
    """-> ([n, D] float32 view that starts offset_words floats into its (16-byte aligned) buffer, the scales with zeros)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2.0, 2.0, (n, D)).astype(np.float32)
    x[0, 0], x[-1, D - 1], x[n // 2, 1] = -0.0, np.nan, -0.0
    scale = rng.uniform(0.0, 0.2, D).astype(np.float32)
    scale[rng.choice(D, D // 4, replace=False)] = 0.0
    scale[0], scale[D - 1] = 0.0, 0.1             # a -0.0 under a zero scale, the NaN under a non-zero one
    buf = torch.zeros(n * D + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[offset_words:offset_words + n * D].view(n, D)
    view.copy_(torch.from_numpy(x))
    return view, x, scale


#            D   offset in floats   path
NOISE_SHAPES = [(38, 0, "scalar"), (42, 0, "scalar"), (210, 0, "scalar"), (76, 0, "vector"), (76, 1, "scalar")]


@pytest.mark.parametrize("D,offset,path", NOISE_SHAPES)
@pytest.mark.parametrize("n", SIZES)
def test_noise_kernel_equals_the_host_program_and_the_prediction(gpu_device, exe, n, D, offset, path):
    """Three consecutive calls: the first out of place, the others in place on its output"""
    view, x, scale = _rows(n, D, offset, 100 * D + n)
    assert (view.data_ptr() % 16 == 0 and D % 4 == 0) == (path == "vector")
    ts = torch.from_numpy(scale).to(DEV)
    count = torch.zeros(n, dtype=torch.int32, device=DEV)
    out = torch.full((n, D), 7.0, dtype=torch.float32, device=DEV)
    if offset:
        out = torch.zeros(n * D + 4, dtype=torch.float32, device=DEV)[offset:offset + n * D].view(n, D)
    cur, cnt = x, np.zeros(n, dtype=np.uint32)
    for call in range(3):
        if call == 0:
            got = channel.obs_noise(SEED, OFF, ts, count, view, out=out)
        else:
            got = channel.obs_noise(SEED, OFF, ts, count, out)
            assert got.data_ptr() == out.data_ptr()
        g = got.cpu().numpy()
        want, cnt = cu.noise_rows(SEED, OFF, cnt, scale, cur)
        assert np.array_equal(cu.bits32(g), cu.bits32(want)), (n, D, offset, call)
        host = cu.host_noise(exe, [(SEED, OFF + i, call, scale, cur[i], call > 0) for i in range(n)])
        assert np.array_equal(cu.bits32(g), np.stack([h[0] for h in host])), (n, D, offset, call)
        assert np.array_equal(count.cpu().numpy().view(np.uint32), cnt) and np.all(cnt == call + 1)
        cur = g
    assert np.array_equal(cu.bits32(view.cpu().numpy()), cu.bits32(x))                  # the input of the out-of-place call is untouched
    zero = scale == 0.0
    assert np.array_equal(cu.bits32(cur)[:, zero], cu.bits32(x)[:, zero]) and not np.array_equal(cu.bits32(cur)[:, ~zero], cu.bits32(x)[:, ~zero])


@pytest.mark.parametrize("D,offset", [(42, 0), (76, 0)])
def test_masked_rows_and_their_counts_are_untouched(gpu_device, D, offset):
    n = 65
    view, x, scale = _rows(n, D, offset, 7)
    ts = torch.from_numpy(scale).to(DEV)
    count = torch.arange(n, dtype=torch.int32, device=DEV)                  # every row at a count of its own
    mask = (torch.arange(n, device=DEV) % 2 == 0)
    view[1::2] = float("nan")                                              # the masked rows: a pattern any arithmetic would change
    before = cu.bits32(view.cpu().numpy())
    channel.obs_noise(SEED, OFF, ts, count, view, mask=mask)
    want, cnt = cu.noise_rows(SEED, OFF, np.arange(n), scale, before.view(np.float32), mask=mask.cpu().numpy())
    got = cu.bits32(view.cpu().numpy())
    assert np.array_equal(got, cu.bits32(want)) and np.array_equal(got[1::2], before[1::2])
    assert np.array_equal(count.cpu().numpy().view(np.uint32), cnt) and np.array_equal(cnt[1::2], np.arange(n)[1::2])
    out = torch.full((n, D), 7.0, device=DEV)
    channel.obs_noise(SEED, OFF, ts, count, view, out=out, mask=mask.to(torch.uint8))
    assert bool((out[1::2] == 7.0).all())                                  # out of place too: a masked row is not written


@pytest.mark.parametrize("D", [42, 76])
def test_two_shards_equal_one_batch(gpu_device, D):
    view, x, scale = _rows(130, D, 0, 9)
    ts = torch.from_numpy(scale).to(DEV)
    whole, a, b = view.clone(), view[:65].clone(), view[65:].clone()
    cw, ca, cb = (torch.zeros(k, dtype=torch.int32, device=DEV) for k in (130, 65, 65))
    for _ in range(2):
        channel.obs_noise(SEED, OFF, ts, cw, whole)
        channel.obs_noise(SEED, OFF, ts, ca, a)
        channel.obs_noise(SEED, OFF + 65, ts, cb, b)
    assert np.array_equal(cu.bits32(whole.cpu().numpy()), cu.bits32(torch.cat([a, b]).cpu().numpy()))
    assert not torch.equal(whole[:65], whole[65:])


def _act_inputs(n, A):
    T = len(RESTARTS)
    actions = np.random.default_rng(n + A).uniform(-1.0, 1.0, (T, n, A)).astype(np.float32)
    restart = np.array([[0 if t == 0 else RESTARTS[(t + i) % T] for i in range(n)] for t in range(T)], dtype=np.uint8)
    return actions, restart


@pytest.mark.parametrize("A,lo,hi,r", ACT_CASES)
def test_actuate_kernel_equals_the_host_program_and_the_prediction(gpu_device, exe, A, lo, hi, r):
    """12 calls over zeroed memory, call 0 with restart == NULL, every env on a restart pattern of its own; actions_out and the whole
    memory rows after every call.  The (12, 0, 4, 0.2) case runs in place."""
    T = len(RESTARTS)
    in_place = (A, lo, hi, r) == (12, 0, 4, 0.2)
    seen_latency = set()
    for n in SIZES:
        actions, restart = _act_inputs(n, A)
        p = channel.make_actuation(SEED, OFF, A, (lo, hi), r)
        mem = channel.ActuatorMem(n, DEV)
        ref = cu.Actuator(SEED, OFF, n, A, lo, hi, r)
        flags = ["".join("-" if t == 0 else str(int(restart[t, i])) for t in range(T)) for i in range(n)]
        host_out, host_rows = cu.host_actuate_many(exe, SEED, [OFF + i for i in range(n)], A, lo, hi, r, actions.transpose(1, 0, 2), flags)
        for t in range(T):
            a = torch.from_numpy(actions[t]).to(DEV)
            rs = None if t == 0 else torch.from_numpy(restart[t]).to(DEV)
            out = channel.actuate(p, mem, a, out=a if in_place else None, restart=rs)
            assert (out.data_ptr() == a.data_ptr()) == in_place
            if not in_place:
                assert np.array_equal(cu.bits32(a.cpu().numpy()), cu.bits32(actions[t]))        # the raw actions are never written
            want = ref.call(actions[t], None if t == 0 else restart[t])
            got, rows = cu.bits32(out.cpu().numpy()), mem.data.cpu().numpy().view(np.uint32)
            assert np.array_equal(got, cu.bits32(want)) and np.array_equal(got, host_out[:, t]), (n, t)
            assert np.array_equal(rows, ref.rows()) and np.array_equal(rows, host_rows[:, t]), (n, t)
        seen_latency |= set(ref.latency.tolist())
        assert np.array_equal(mem.episodes.cpu().numpy(), 1 + restart[1:].sum(0))
    assert seen_latency == set(range(lo, hi + 1))


# ---- twin handles
def _cfg(episode_length=10):
    c = default_config(ROBOT_SOLO12, TASK_WALK)
    c.num_history_stack = 1
    c.episode_length = episode_length
    return c


def _env(N, seed=5, off=3, **kw):
    from solorl_amd.vec_env import SoloVecEnv
    return SoloVecEnv(_cfg(), N, device=DEV, seed=seed, env_id_offset=off, **kw)


def _actions(N, steps, seed=11):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    return [(torch.rand(N, 12, device=DEV, generator=g) * 2 - 1).contiguous() for _ in range(steps)]


GROUPS = {"height": 0.01, "orientation": 0.03, "lin_vel": 0.1, "ang_vel": 0.2, "joint_pos": 0.01, "joint_vel": 1.5}


def _same_info(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("N", (6, 130))
def test_noise_changes_the_observations_and_nothing_else(gpu_device, N):
    A, B = _env(N), _env(N)
    A.set_obs_noise(dict(groups=GROUPS, history=0.5))
    scale = channel.noise_scales(A.cfg, GROUPS, history=0.5).numpy()
    assert np.array_equal(A._noise_scale.cpu().numpy(), scale) and (scale[:76] > 0).sum() == 2 * 34
    cnt = np.zeros(N, dtype=np.uint32)
    oa, ob = A.reset(), B.reset()
    want, cnt = cu.noise_rows(5, 3, cnt, scale, ob.cpu().numpy())
    assert np.array_equal(cu.bits32(oa.cpu().numpy()), cu.bits32(want)) and not torch.equal(oa, ob)
    resets = 0
    for t, act in enumerate(_actions(N, 30)):
        if t % 2:
            (oa, ra, da, ia), (ob, rb, db, ib) = A.step_inplace(act), B.step_inplace(act)
        else:
            (oa, ra, da, la), (ob, rb, db, lb) = A.step(act), B.step(act)
            ia, ib = la.tensors, lb.tensors
        assert torch.equal(ra, rb) and torch.equal(da, db) and _same_info(ia, ib), t        # rewards, done flags and info: the plain twin's
        want, cnt = cu.noise_rows(5, 3, cnt, scale, ob.cpu().numpy())
        assert np.array_equal(cu.bits32(oa.cpu().numpy()), cu.bits32(want)), t
        resets += int(db.sum())
    assert resets >= 2 * N                                                              # auto-resets occurred (episode_length 10)
    assert torch.equal(A.get_observation(), B.get_observation())                        # get_observation() stays clean
    assert np.array_equal(A._noise_count.cpu().numpy().view(np.uint32), cnt) and np.all(cnt == 31)
    # reset_masked: the selected rows are noisy reset observations, the others the clean current ones; only the selected counts advance
    mask = torch.arange(N, device=DEV) % 3 == 0
    oa, ob = A.reset_masked(mask), B.reset_masked(mask)
    want, cnt = cu.noise_rows(5, 3, cnt, scale, ob.cpu().numpy(), mask=mask.cpu().numpy())
    assert np.array_equal(cu.bits32(oa.cpu().numpy()), cu.bits32(want)) and torch.equal(oa[~mask], ob[~mask])
    assert np.array_equal(A._noise_count.cpu().numpy().view(np.uint32), cnt)
    A.close(); B.close()


@pytest.mark.parametrize("N", (6, 130))
def test_actuation_is_the_twin_stepped_with_the_predicted_applied_actions(gpu_device, N):
    A, B = _env(N), _env(N)
    A.set_actuation((0, 3), 0.2)
    ref = cu.Actuator(5, 3, N, 12, 0, 3, 0.2)
    oa, ob = A.reset(), B.reset()
    assert torch.equal(oa, ob)
    restart = np.ones(N, dtype=np.uint8)
    delayed = 0
    for t, act in enumerate(_actions(N, 30)):
        if t == 15:                                       # a reset_masked in the middle restarts exactly the masked envs
            mask = torch.arange(N, device=DEV) % 3 == 1
            assert torch.equal(A.reset_masked(mask), B.reset_masked(mask))
            restart = restart | mask.cpu().numpy().astype(np.uint8)
            before = ref.episodes.copy()
        raw = act.clone()
        applied = ref.call(act.cpu().numpy(), restart)
        if t == 15:
            assert np.array_equal(ref.episodes - before, restart)
        oa, ra, da, ia = A.step_inplace(act)
        ob, rb, db, ib = B.step_inplace(torch.from_numpy(applied).to(DEV))
        assert np.array_equal(cu.bits32(A.last_applied_actions.cpu().numpy()), cu.bits32(applied)), t
        assert torch.equal(act, raw)                      # the caller's tensor is never written
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db) and _same_info(ia, ib), t
        assert np.array_equal(A._act_mem.data.cpu().numpy().view(np.uint32), ref.rows()), t
        restart = db.cpu().numpy().copy()                 # the plain twin's own done flags
        delayed += int((cu.bits32(applied) != cu.bits32(act.cpu().numpy())).any(axis=1).sum())
    assert delayed > 20 * N and set(ref.latency.tolist()) == {0, 1, 2, 3}
    A.close(); B.close()


def test_a_captured_step_with_both_features_equals_an_eager_twin(gpu_device):
    N = 130
    A, B = _env(N), _env(N)
    for e in (A, B):
        e.set_obs_noise(GROUPS)
        e.set_actuation((0, 3), 0.2)                      # (both allocate here: before the capture)
        e.reset()
    act = torch.zeros(N, 12, device=DEV)
    acts = _actions(N, 6, seed=21)
    act.copy_(acts[0])
    oa, ra, da, _ = A.step_inplace(act)                   # a warm-up step on both
    ob, rb, db, _ = B.step_inplace(acts[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa, ra, da, _ = A.step_inplace(act)
    for r in range(5):
        act.copy_(acts[1 + r])
        graph.replay()
        ob, rb, db, _ = B.step_inplace(acts[1 + r])
        torch.cuda.synchronize()
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), r
        assert torch.equal(A.last_applied_actions, B.last_applied_actions) and torch.equal(A._act_mem.data, B._act_mem.data)
        assert torch.equal(A._noise_count, B._noise_count) and int(A._noise_count[0]) == 3 + r
    assert np.array_equal(A.get_states().bytes().cpu().numpy(), B.get_states().bytes().cpu().numpy())
    A.close(); B.close()


def _random_policy(O=76, A=12, seed=3):
    from solorl_amd.ppo import Policy
    from solorl_amd.vec_env import Box
    torch.manual_seed(seed)
    pol = Policy((O,), Box(-np.ones(A), np.ones(A)), None, {"hidden_size": 64}).to(DEV)
    with torch.no_grad():
        pol.pi_dist.logstd.normal_(0, 0.3)
        for p in pol.parameters():
            if p.dim() == 1 and p is not pol.pi_dist.logstd:
                p.normal_(0, 0.1)
    return pol


def test_policy_tail_with_actuation_and_not_with_noise(gpu_device):
    """step_act_inplace with actuation = step_inplace + solorl_policy_act on a twin: observations, rewards and done flags bitwise, value,
    action and log-prob within 2e-6 of 1 + |value| (the separate kernel sums in another order); the tail's raw action is delayed at the
    next call.  One run on an MI355X: 5.2e-7 (value), 6.3e-7 (action), 1.9e-7 (log-prob)."""
    from solorl_amd.ppo.fused import policy_act, policy_params
    N = 67
    P = policy_params(_random_policy())
    A, B = _env(N), _env(N)
    assert A.step_act_supported(P) and A.rollout_supported(P)
    for e in (A, B):
        e.set_actuation((0, 3), 0.2)
    assert A.step_act_supported(P) and not A.rollout_supported(P)             # True with actuation alone (K steps in one launch: no)
    A.reset(); B.reset()
    g = torch.Generator(device=DEV); g.manual_seed(5)
    act = torch.rand(N, 12, device=DEV, generator=g) * 2 - 1
    worst = dict(v=0.0, a=0.0, l=0.0)
    for t in range(12):
        noise = torch.randn(N, 12, device=DEV, generator=g) if t % 3 else None
        o1, r1, d1, _ = B.step_inplace(act)
        v1, a1, l1 = torch.empty(N, 1, device=DEV), torch.empty(N, 12, device=DEV), torch.empty(N, 1, device=DEV)
        policy_act(P, o1, noise, v1, a1, l1)
        v2, a2, l2 = torch.full((N, 1), 7.0, device=DEV), torch.full((N, 12), 7.0, device=DEV), torch.full((N, 1), 7.0, device=DEV)
        o2, r2, d2, _ = A.step_act_inplace(act, P, noise, v2, a2, l2)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2), t
        assert torch.equal(A.last_applied_actions, B.last_applied_actions) and torch.equal(A._act_mem.data, B._act_mem.data)
        for k, x, y in (("v", v1, v2), ("a", a1, a2), ("l", l1, l2)):
            worst[k] = max(worst[k], float(((x - y).abs() / (1.0 + y.abs())).max()))
        act = a2.clone()                                  # closed loop: the tail's raw action, delayed at the next call
    print("step_act_inplace with actuation against step_inplace + policy_act:", worst)
    assert worst["v"] < 2e-6 and worst["a"] < 2e-6 and worst["l"] < 2e-6, worst
    A.set_obs_noise(GROUPS)
    assert not A.step_act_supported(P) and not A.rollout_supported(P)         # False with noise
    with pytest.raises(_native.SoloRLError, match="observation noise"):
        A.step_act_inplace(act, P, None, v2, a2, l2)
    A.set_obs_noise(None); A.set_actuation(None)
    assert A.step_act_supported(P) and A.rollout_supported(P)
    A.close(); B.close()


def test_refusals_and_the_off_state(gpu_device):
    from solorl_amd.ppo.fused import policy_params
    from solorl_amd.vec_env import make_vec_envs
    N = 8
    P = policy_params(_random_policy())
    env = _env(N)
    off = ("_noise_scale", "_noise_count", "_act", "_act_mem", "_act_restart", "last_applied_actions")
    assert all(getattr(env, k) is None for k in off)                          # off: nothing is allocated
    env.reset()
    acts = torch.zeros(2, N, 12, device=DEV)
    val, lp = torch.zeros(2, N, device=DEV), torch.zeros(2, N, device=DEV)
    env.step_n_inplace(acts)
    env.rollout_inplace(acts, P, None, val, lp)
    assert all(getattr(env, k) is None for k in off)
    for on, clear in ((lambda: env.set_obs_noise(GROUPS), lambda: env.set_obs_noise(None)),
                      (lambda: env.set_actuation(2), lambda: env.set_actuation(None)),
                      (lambda: env.set_actuation(None, 0.1), lambda: env.set_actuation(None, 0.0))):
        on()
        with pytest.raises(_native.SoloRLError, match="step_n"):
            env.step_n_inplace(acts)
        with pytest.raises(_native.SoloRLError, match="step_n"):
            env.step_n(acts)
        with pytest.raises(_native.SoloRLError, match="rollout_inplace"):
            env.rollout_inplace(acts, P, None, val, lp)
        clear()
        assert all(getattr(env, k) is None for k in off)
        env.step_n_inplace(acts)                                              # allowed again
    with pytest.raises(AssertionError):
        env.set_obs_noise(torch.zeros(75))
    with pytest.raises(ValueError, match="hieght"):
        env.set_obs_noise({"hieght": 0.1})
    with pytest.raises(AssertionError):
        env.set_actuation((0, 5))
    with pytest.raises(AssertionError):
        env.set_actuation(1, 1.0)
    assert all(getattr(env, k) is None for k in off)
    env.set_obs_noise(torch.full((76,), 0.01))                                # an [obs_dim] vector
    assert tuple(env._noise_scale.shape) == (76,) and env._noise_scale.is_cuda
    env.close()
    plain = make_vec_envs(dict(episode_length=10, solo12=True, task="walk", num_history_stack=1), N, device=DEV)
    assert all(getattr(plain, k) is None for k in off)
    plain.close()
    both = make_vec_envs(dict(episode_length=10, solo12=True, task="walk", num_history_stack=1), N, device=DEV, obs_noise=dict(groups=GROUPS),
                         action_delay=(0, 2), motor_gain_range=0.1)
    assert both._noise_scale is not None and (both._act.delay_min, both._act.delay_max, both._act.gain_range) == (0, 2, 0.1)
    both.close()


# ---- training and evaluation with the three flags
T_STEPS, N_TRAIN, UPDATES = 16, 64, 2


def _train(monkeypatch, graphs):
    """train() for two updates of 64 walk12 envs x 16 steps with the three flags -> (the env, the GraphedRollout or None, the history)"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import train_ppo
    from solorl_amd import vec_env
    from solorl_amd.ppo import train as tr
    from solorl_amd.config import load_yaml
    argv = ["--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", str(N_TRAIN), "--num-steps", str(T_STEPS),
            "--num-env-steps", str(N_TRAIN * T_STEPS * UPDATES), "--mini-batch-size", "512", "--ppo-epoch", "2", "--use-gae", "--seed", "7", "--log-interval", "1",
            "--obs-noise", os.path.join(ROOT, "configs", "noise_solo.yaml"), "--action-delay", "0:3", "--motor-gain-range", "0.2"]
    if not graphs:
        argv += ["--no-hip-graphs"]
    args = train_ppo.get_ppo_args(argv)
    args.cuda = True
    config = load_yaml(args.config_file)
    config["task"] = args.task
    args.obs_noise = train_ppo.load_obs_noise(args.obs_noise, config)
    seen = {}
    make, Graphed = vec_env.make_vec_envs, tr.GraphedRollout

    def keep(name, f):
        def g(*a, **k):
            seen[name] = f(*a, **k)
            return seen[name]
        return g
    monkeypatch.setattr(vec_env, "make_vec_envs", keep("env", make))
    monkeypatch.setattr(tr, "GraphedRollout", keep("graphed", Graphed))
    pol, hist = tr.train(args, config)
    torch.cuda.synchronize()
    assert len(hist) == UPDATES and all(torch.isfinite(p).all() for p in pol.parameters())
    return seen["env"], seen.get("graphed"), hist


@pytest.mark.parametrize("graphs", (True, False), ids=("hip_graphs", "eager"))
def test_training_with_the_three_flags(gpu_device, monkeypatch, graphs):
    monkeypatch.delenv("SOLORL_ROLLOUT_CHUNK", raising=False)
    env, graphed, hist = _train(monkeypatch, graphs)
    for rec in hist:
        assert all(math.isfinite(float(rec[k])) for k in rec if "loss" in k or k == "entropy"), rec
        assert any("loss" in k for k in rec), rec
    if graphs:
        assert graphed is not None and graphed.graph is not None and graphed.step_act is False      # the two-launch path, on its own
    else:
        assert graphed is None
    # reset() and every rollout step drew noise once; every step went through the actuator
    assert np.all(env._noise_count.cpu().numpy() == 1 + UPDATES * T_STEPS)
    assert int(env._act_mem.episodes.min()) >= 1 and set(env._act_mem.latency.unique().tolist()) <= {0, 1, 2, 3}
    assert not torch.equal(env.last_applied_actions, torch.zeros_like(env.last_applied_actions))


def test_eval_ppo_with_the_three_flags(gpu_device, tmp_path):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import eval_ppo
    sd = torch.load(os.path.join(ROOT, "tests", "golden", "policies", "walk12.pt"), map_location="cpu", weights_only=False)
    torch.save({"update": 0, "state_dict": sd, "ob_rms": None}, os.path.join(str(tmp_path), "solo.pt"))
    base = ["--checkpoint-dir", str(tmp_path), "--config-file", os.path.join(ROOT, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", "16",
            "--num-runs", "4", "--deterministic"]
    plain = eval_ppo.main(base)
    r = eval_ppo.main(base + ["--obs-noise", os.path.join(ROOT, "configs", "noise_solo.yaml"), "--action-delay", "1:2", "--motor-gain-range", "0.1"])
    print("walk12 fixture, plain:", plain, "with noise, delay 1..2 and 10 % gain error:", r)
    assert plain["episodes"] >= 4 and r["episodes"] >= 4
    assert all(math.isfinite(float(r[k])) for k in ("mean_length", "mean_reward", "mean_success"))
    assert 1 <= r["mean_length"] <= 400 and 0.0 <= r["mean_success"] <= 1.0 and r != plain
