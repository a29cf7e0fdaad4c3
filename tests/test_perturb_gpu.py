"""Device-side kicks on the GPU (include/solorl.h solorl_set_perturbation / solorl_perturb / solorl_get_perturbation; SoloVecEnv
set_perturbation, perturb, last_kick, perturbation_state; train_ppo.py --push-interval).

Prediction: tests/perturb_util.py -- the oracle's Philox and the draw table of the header, nothing of the engine.  Kicks are compared
bitwise, countdowns and counts exactly.

Shapes: N = 6 (two slot groups of four, the last one half full) and N = 130 (several team workgroups, a partial 64-lane wavefront); the
kernel runs one thread per env in blocks of 256, so N = 258 (a second block with two threads) for the fp32 team case.  Handle forms and
the _make / _prepared helpers are those of tests/test_states_gpu.py; where two handles are stepped side by side the sorted team-mode
case is left out for the reason that file's docstring gives (a team-mode env's last bits depend on its wavefront's slot set).

A control step of a handle with a perturbation set is  kick -> physics:  step_inplace() issues solorl_perturb itself, right before its
step launch, so "(perturb, step_inplace)" below is one step_inplace() call; perturb() alone is the explicit call, without a step."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from solorl_amd import _native
from solorl_amd.config import (default_config, ROBOT_SOLO8, ROBOT_SOLO12, TASK_STAND, TASK_WALK, TASK_POINTGOAL,
                               PRECISION_F64)
from tests import perturb_util as pu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (6, 130)
#        name                  robot         task            f64  H  environment
CASES = {"walk12":             (ROBOT_SOLO12, TASK_WALK,      0, 1, {}),
         "stand8":             (ROBOT_SOLO8,  TASK_STAND,     0, 0, {}),
         "pointgoal12_f64":    (ROBOT_SOLO12, TASK_POINTGOAL, 1, 3, {}),
         "walk12_sorted_lane": (ROBOT_SOLO12, TASK_WALK,      0, 1, {"SOLORL_SORT": "1", "SOLORL_TEAM": "0"}),
         "walk12_lane":        (ROBOT_SOLO12, TASK_WALK,      0, 1, {"SOLORL_TEAM": "0"}),
         "walk12_sorted_team": (ROBOT_SOLO12, TASK_WALK,      0, 1, {"SOLORL_SORT": "1"})}
ALL_CASES = tuple(CASES)
TWIN_STEP_CASES = tuple(c for c in CASES if c != "walk12_sorted_team")
CASE_SIZES = [(c, n) for c in ALL_CASES for n in SIZES] + [("walk12", 258)]
SEED, OFF = 5, 3
INTERVAL = (2, 5)
LIN, ANG = (0.5, 0.3, 0.2), (0.4, 0.6, 1.0)


def _cfg(case):
    robot, task, f64, H, _ = CASES[case]
    c = default_config(robot, task)
    c.num_history_stack = H
    if f64:
        c.precision = PRECISION_F64
    return c


def _make(case, N, monkeypatch, seed=SEED, off=OFF):
    from solorl_amd.vec_env import SoloVecEnv
    for k in ("SOLORL_SORT", "SOLORL_TEAM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in CASES[case][4].items():
        monkeypatch.setenv(k, v)                     # (read at solorl_create)
    return SoloVecEnv(_cfg(case), N, device=DEV, seed=seed, env_id_offset=off)


def _actions(N, A, steps, seed=11):
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    return [(torch.rand(N, A, device=DEV, generator=g) * 2 - 1).contiguous() for _ in range(steps)]


def _prepared(case, N, monkeypatch, seed=SEED, steps=5, act_seed=11, off=OFF):
    env = _make(case, N, monkeypatch, seed, off)
    env.reset()
    for a in _actions(N, env.act_dim, steps, act_seed):
        env.step_inplace(a)
    return env


def _rows(sb):
    return sb.bytes().cpu().numpy()


def _kick_bits(env):
    return pu.bits(env.last_kick.cpu().numpy())


def _sched(env):
    cd, kc = env.perturbation_state()
    return cd.cpu().numpy(), kc.cpu().numpy()


@pytest.mark.parametrize("case,N", CASE_SIZES)
def test_draws_equal_the_prediction(gpu_device, monkeypatch, case, N):
    """12 x (perturb, step_inplace): after every call last_kick and perturbation_state() are the prediction's; every env is kicked at
    least twice (12 calls, intervals of at most 5); no perturb call changes a row's rng_counter, and (TWIN_STEP_CASES) the rng_counter of
    every env equals that of a twin handle without perturbation after every step.  The twin is given the same kicks through push():
    rng_counter advances at every reset, and a twin that is not kicked at all falls -- and resets -- at other steps than the kicked
    handle (seen on the device: env 4 of walk12, N = 6 terminated at step 9 of the un-kicked twin only), which says nothing about the
    kicks' draws.  Pushed alike, the two handles reset at the same steps, and their counters differ exactly if a kick advanced one."""
    env = _prepared(case, N, monkeypatch)
    twin = _prepared(case, N, monkeypatch) if case in TWIN_STEP_CASES else None
    env.set_perturbation(INTERVAL, LIN, ANG)
    want = pu.Schedule(SEED, OFF, N, INTERVAL, LIN + ANG)
    cd, kc = _sched(env)
    assert np.array_equal(cd, want.countdown) and not kc.any()
    assert cd.min() >= INTERVAL[0] and cd.max() <= INTERVAL[1]
    for t, a in enumerate(_actions(N, env.act_dim, 12, seed=23)):
        rng0 = env.get_states().rng_counter.clone()
        k = env.perturb() if t % 2 else None           # odd calls: the explicit call and a step on a handle whose step does not kick ...
        if k is not None:
            assert torch.equal(env.get_states().rng_counter, rng0)
            lk, env.last_kick = env.last_kick, None    # (... by taking the vec-env's switch away for the one step call)
            env.step_inplace(a)
            env.last_kick = lk
        else:                                          # even calls: step_inplace issues the kick itself
            env.step_inplace(a)
        kick = want.call()
        assert np.array_equal(_kick_bits(env), pu.bits(kick)), (case, N, t)
        cd, kc = _sched(env)
        assert np.array_equal(cd, want.countdown) and np.array_equal(kc, want.kicks), (case, N, t)
        if twin is not None:
            twin.push(env.last_kick, torch.from_numpy(kick.any(axis=1)).to(DEV))
            twin.step_inplace(a)
            assert torch.equal(env.get_states().rng_counter, twin.get_states().rng_counter), (case, N, t)
    assert want.kicks.min() >= 2


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("case", ("walk12", "walk12_lane", "pointgoal12_f64"))
def test_perturb_equals_push_with_the_same_kick(gpu_device, monkeypatch, case, N):
    """A is kicked by the engine, B by push(A.last_kick, mask = the envs A kicked): get_states bitwise equal after each of 6 steps.  All
    six amplitudes are non-zero, so no component meets the zero-amplitude rule."""
    A, B = _prepared(case, N, monkeypatch), _prepared(case, N, monkeypatch)
    A.set_perturbation(INTERVAL, LIN, ANG)
    kicked_any = 0
    for t, a in enumerate(_actions(N, A.act_dim, 6, seed=31)):
        before = A.perturbation_state()[1]
        A.step_inplace(a)                              # kick -> physics
        kicked = A.perturbation_state()[1] != before
        kicked_any += int(kicked.sum())
        B.push(A.last_kick, kicked)
        B.step_inplace(a)
        assert np.array_equal(_rows(A.get_states()), _rows(B.get_states())), (case, N, t)
    assert kicked_any >= N                             # (intervals of at most 5: every env within 6 steps)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("case", TWIN_STEP_CASES)
def test_zero_amplitudes_are_exact_no_ops_over_steps(gpu_device, monkeypatch, case, N):
    """All amplitudes 0, a kick due in every step, against a handle that never set a perturbation: states, observations, rewards and
    done flags bitwise equal over 8 steps, last_kick all (+0.0) zeros."""
    A, B = _prepared(case, N, monkeypatch), _prepared(case, N, monkeypatch)
    A.set_perturbation(1, 0.0, 0.0)
    for t, a in enumerate(_actions(N, A.act_dim, 8, seed=37)):
        oa, ra, da, _ = A.step_inplace(a)
        ob, rb, db, _ = B.step_inplace(a)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), (case, N, t)
        assert np.array_equal(_rows(A.get_states()), _rows(B.get_states())), (case, N, t)
        assert not _kick_bits(A).any()
    assert (A.perturbation_state()[1] == 8).all()      # every call did draw a kick


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("case", ALL_CASES)
def test_zero_amplitude_components_are_not_written(gpu_device, monkeypatch, case, N):
    """Amplitudes lin (0.5, 0, 0): a perturb call that kicks every env leaves lin_vel[1:] and ang_vel -- set to -0.0 beforehand, which
    v + 0.0 would turn into +0.0 -- and every other word of the rows as they were; lin_vel[0] is T(double(v) + kick)."""
    env = _prepared(case, N, monkeypatch)
    s = env.get_states()
    s.lin_vel[:, 1:] = -0.0
    s.ang_vel[:] = -0.0
    env.set_states(s, fields="vel")
    env.set_perturbation(1, (0.5, 0.0, 0.0), 0.0)
    before = env.get_states()
    kick = env.perturb().clone()
    after = env.get_states()
    want_kick = pu.Schedule(SEED, OFF, N, (1, 1), (0.5, 0, 0, 0, 0, 0)).call()
    assert np.array_equal(pu.bits(kick.cpu().numpy()), pu.bits(want_kick)) and np.count_nonzero(want_kick[:, 0]) >= N - 1
    neg0 = np.uint64(1) << np.uint64(63)
    assert (pu.bits(after.lin_vel[:, 1:].cpu().numpy()) == neg0).all() and (pu.bits(after.ang_vel.cpu().numpy()) == neg0).all()
    vx = before.lin_vel[:, 0] + kick[:, 0]
    if not CASES[case][2]:
        vx = vx.float().double()                       # an fp32 engine rounds the sum to float once
    want = before.clone()
    want.lin_vel[:, 0] = vx
    assert np.array_equal(_rows(after), _rows(want))


def test_error_codes(gpu_device, monkeypatch):
    N = 6
    env = _make("walk12", N, monkeypatch)
    L, h = env.L, env._h
    ERR_INVALID, ERR_STATE = -1, -4
    assert L.solorl_perturb(h, None, None) == ERR_STATE and b"solorl_perturb" in L.solorl_last_error()      # nothing set
    good = _native.Perturbation(2, 5, (C.c_double * 3)(0.5, 0.5, 0.0), (C.c_double * 3)(0.0, 0.0, 0.5))
    assert L.solorl_set_perturbation(h, C.byref(good)) == 0
    assert L.solorl_perturb(h, None, None) == ERR_STATE and b"solorl_perturb" in L.solorl_last_error()      # set, but never reset
    env.reset()
    assert L.solorl_perturb(h, None, None) == 0
    for imin, imax, lin, ang in ((0, 5, (0.5, 0, 0), (0, 0, 0)), (5, 4, (0.5, 0, 0), (0, 0, 0)), (2, 5, (0.5, -0.1, 0), (0, 0, 0)),
                                 (2, 5, (0.5, 0, 0), (0, float("nan"), 0)), (2, 5, (float("inf"), 0, 0), (0, 0, 0))):
        bad = _native.Perturbation(imin, imax, (C.c_double * 3)(*lin), (C.c_double * 3)(*ang))
        assert L.solorl_set_perturbation(h, C.byref(bad)) == ERR_INVALID, (imin, imax, lin, ang)
        assert b"solorl_set_perturbation" in L.solorl_last_error()
    assert L.solorl_perturb(h, None, None) == 0                       # a refused call leaves the perturbation as it was
    cd = torch.empty(N, dtype=torch.int32, device=DEV)
    assert L.solorl_get_perturbation(h, C.c_void_p(cd.data_ptr()), None, None) == 0
    assert L.solorl_get_perturbation(h, None, None, None) == ERR_INVALID
    assert L.solorl_set_perturbation(h, None) == 0                     # off
    assert L.solorl_perturb(h, None, None) == ERR_STATE
    assert L.solorl_get_perturbation(h, C.c_void_p(cd.data_ptr()), None, None) == ERR_STATE
    # the vec-env: K steps in one launch cannot take kicks
    env.set_perturbation((2, 5), 0.5)
    acts = torch.zeros(2, N, env.act_dim, device=DEV)
    with pytest.raises(_native.SoloRLError, match="perturbation"):
        env.step_n(acts)
    with pytest.raises(_native.SoloRLError, match="perturbation"):
        env.step_n_inplace(acts)
    with pytest.raises(_native.SoloRLError, match="perturbation"):
        env.rollout_inplace(acts, None, None, None, None)
    assert env.rollout_supported(None) is False
    env.set_perturbation(None)
    assert env.last_kick is None
    with pytest.raises(_native.SoloRLError, match="solorl error -4"):
        env.perturb()
    env.step_n_inplace(acts)                                           # allowed again
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", ("walk12", "pointgoal12_f64"))
def test_shards_kick_like_one_batch(gpu_device, monkeypatch, case):
    """Draws are keyed by global env id: handles of 6 envs at offsets 3 and 9 against one of 12 at offset 3, 10 perturb calls each."""
    parts = [_make(case, 6, monkeypatch, off=3), _make(case, 6, monkeypatch, off=9)]
    whole = _make(case, 12, monkeypatch, off=3)
    for e in parts + [whole]:
        e.reset()
        e.set_perturbation(INTERVAL, LIN, ANG)
    total = 0
    for t in range(10):
        ks = [e.perturb().cpu().numpy() for e in parts]
        kw = whole.perturb().cpu().numpy()
        assert np.array_equal(pu.bits(np.concatenate(ks)), pu.bits(kw)), (case, t)
        total += np.count_nonzero(kw)
    assert total >= 12 * 2 * 6
    for a, b in zip(zip(*[_sched(e) for e in parts]), _sched(whole)):
        assert np.array_equal(np.concatenate(a), b)


@pytest.mark.parametrize("case,N", [("walk12", 6), ("walk12", 130), ("walk12_sorted_lane", 130)])
def test_perturb_and_step_are_capturable(gpu_device, monkeypatch, case, N):
    """One graph of 6 x (perturb, step_inplace) replayed twice against 12 eager pairs on a twin (an even number of steps: a sorted handle
    is back on the state buffer the graph starts from): states, last_kick and perturbation_state() bitwise equal after each replay."""
    A, B = _prepared(case, N, monkeypatch), _prepared(case, N, monkeypatch)
    for e in (A, B):
        e.set_perturbation(INTERVAL, LIN, ANG)         # (allocates last_kick: before the capture)
    gen = torch.Generator(device=DEV); gen.manual_seed(41)
    act = torch.zeros(6, N, A.act_dim, device=DEV)

    def calls(e):
        for t in range(6):
            out = e.step_inplace(act[t])               # = perturb + step
        return out

    graph = torch.cuda.CUDAGraph()
    kick_ptr = A.last_kick.data_ptr()
    with torch.cuda.graph(graph):
        oa, ra, da, _ = calls(A)
    torch.cuda.synchronize()
    assert A.last_kick.data_ptr() == kick_ptr
    assert np.array_equal(_rows(A.get_states()), _rows(B.get_states())) and not A.perturbation_state()[1].any()      # capturing ran nothing
    want = pu.Schedule(SEED, OFF, N, INTERVAL, LIN + ANG)
    for r in range(2):
        act.copy_(torch.rand(6, N, A.act_dim, device=DEV, generator=gen) * 2 - 1)
        graph.replay()
        ob, rb, db, _ = calls(B)
        for _ in range(6):
            kick = want.call()
        torch.cuda.synchronize()
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), (case, N, r)
        assert np.array_equal(_rows(A.get_states()), _rows(B.get_states())), (case, N, r)
        assert np.array_equal(_kick_bits(A), _kick_bits(B)) and np.array_equal(_kick_bits(A), pu.bits(kick))
        for x, y, z in zip(_sched(A), _sched(B), (want.countdown, want.kicks)):
            assert np.array_equal(x, y) and np.array_equal(x, z)


# ---- training: train_ppo.py --push-interval through make_vec_envs into the eager and the captured rollout
T_STEPS, N_TRAIN, UPDATES = 16, 64, 2


def _train(monkeypatch, graphs, push=True):
    """train() for two updates of 64 walk12 envs x 16 steps -> (the env, the rollout storage, the GraphedRollout or None)"""
    import train_ppo
    from solorl_amd import vec_env
    from solorl_amd.config import load_yaml
    from solorl_amd.ppo import train as tr
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    argv = ["--config-file", os.path.join(root, "configs", "basic12.yaml"), "--task", "walk", "--num-agents", str(N_TRAIN), "--num-steps", str(T_STEPS),
            "--num-env-steps", str(N_TRAIN * T_STEPS * UPDATES), "--mini-batch-size", "512", "--ppo-epoch", "2", "--use-gae", "--seed", "7", "--log-interval", "1"]
    if push:
        argv += ["--push-interval", "3:6", "--push-max-vel", "0.5", "--push-max-yaw-rate", "0.5"]
    if not graphs:
        argv += ["--no-hip-graphs"]
    args = train_ppo.get_ppo_args(argv)
    args.cuda = True
    config = load_yaml(args.config_file)
    config["task"] = args.task
    seen = {}
    make, Storage, Graphed = vec_env.make_vec_envs, tr.RolloutStorage, tr.GraphedRollout

    def keep(name, f):
        def g(*a, **k):
            seen[name] = f(*a, **k)
            return seen[name]
        return g
    monkeypatch.setattr(vec_env, "make_vec_envs", keep("env", make))
    monkeypatch.setattr(tr, "RolloutStorage", keep("storage", Storage))
    monkeypatch.setattr(tr, "GraphedRollout", keep("graphed", Graphed))
    pol, hist = tr.train(args, config)
    torch.cuda.synchronize()
    assert len(hist) == UPDATES and all(torch.isfinite(p).all() for p in pol.parameters())
    return seen["env"], seen["storage"], seen.get("graphed")


def _check_schedule(env):
    """train() steps its envs in the rollouts only -- reset(), then policy calls, no warm-up step (solorl_amd/ppo/train.py: the library
    warm-up in front of the capture is actor_critic.act / get_value on the reset observation) -- so the schedule has advanced by exactly
    UPDATES x T_STEPS calls.  Rank 0's envs are global ids 0 .. N - 1 and the key is --seed."""
    want = pu.Schedule(7, 0, N_TRAIN, (3, 6), (0.5, 0.5, 0.0, 0.0, 0.0, 0.5))
    for _ in range(UPDATES * T_STEPS):
        kick = want.call()
    cd, kc = _sched(env)
    assert np.array_equal(cd, want.countdown) and np.array_equal(kc, want.kicks)
    assert np.array_equal(_kick_bits(env), pu.bits(kick))
    assert want.kicks.min() >= UPDATES * T_STEPS // 6


@pytest.mark.parametrize("graphs", (True, False), ids=("hip_graphs", "eager"))
def test_training_with_pushes(gpu_device, monkeypatch, graphs):
    """Both rollout forms finish and leave the predicted schedule (kick schedules do not depend on actions, so the two agree although
    their noise streams differ: tests/test_train_gpu.py); the stored observations differ from those of a run without the flags."""
    monkeypatch.delenv("SOLORL_ROLLOUT_CHUNK", raising=False)
    env, storage, graphed = _train(monkeypatch, graphs)
    assert (graphed is not None and graphed.graph is not None) if graphs else graphed is None
    _check_schedule(env)
    obs = storage.obs.clone()
    plain_env, plain_storage, _ = _train(monkeypatch, graphs, push=False)
    assert plain_env.last_kick is None
    assert not torch.equal(obs, plain_storage.obs)


def test_training_with_pushes_and_a_rollout_chunk_takes_the_per_step_path(gpu_device, monkeypatch):
    monkeypatch.setenv("SOLORL_ROLLOUT_CHUNK", "4")
    env, storage, graphed = _train(monkeypatch, True)
    assert graphed.chunk == 4 and graphed.windows is None and graphed.graph is not None
    _check_schedule(env)
